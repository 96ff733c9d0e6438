"""Navigation-error (LQG) covariance analysis without a GPU: the independent reference (tests/nav_reference.py: the recursion of
include/scvx.h in numpy with the full T, U and Xi) against the covariance reference it must contain (N0 = 0), against the open-loop
transport (no measurement, zero gains), against its own longdouble form and the properties of a covariance, and against the
nonlinear closed loop of the C oracle flown on sampled estimates; the three bindings (header, _lib.SIGNATURES, julia/ScvxAMD.jl)
against each other; dynamics.NavReport and its argument helpers; montecarlo.measurement_rows / nav_error_samples.

Data: the two plans the oracle converges on (tests/golden/oracle_flight_runs.npz), tiles from oracle.dynamics.linearize."""
import os
import re

import numpy as np
import pytest

import cov_reference as cr
import nav_reference as nr
import track_reference as tr
from conftest import ROOT
from test_cov_cpu import _data

WEIGHTS = [(1.0, 1.0, 100.0), (1.0, 1e-2, 1e4)]


def pv_model(x0):
    """(H, rm) of the checks: position and velocity measured at every node, 1 sigma = 3e-5 of the largest |r| and |v| component of x0"""
    from successiveconvexification_amd.montecarlo import measurement_rows
    H = measurement_rows("rv")
    sd = np.repeat([3e-5 * np.abs(x0[1:4]).max(), 3e-5 * np.abs(x0[4:7]).max()], 3)
    return H, sd * sd


def test_zero_navigation_error_gives_the_covariance_recursion():
    """N0 = 0 and w = 0: eps stays exactly zero, the filter gain is zero, and the z block is cov_reference.propagate's at every node"""
    p, par, x, u, s, d = _data()
    S0 = np.stack([cr.handover_s0(x[b, 0])[0] for b in range(2)])
    H, rm = pv_model(x[0, 0])
    for w in WEIGHTS:
        L, _ = tr.gains(d, p.K, *w)
        cov = cr.propagate(d, p.K, L, S0)
        # 1e-13 relative at the default weights.  Under the stiffer gains float64 itself is no better than that: two float64 evaluations
        # in different summation orders, each within e_ref of the longdouble value, may differ by 2 e_ref (4 e_ref: room for the joint's
        # longer sums)
        cld = cr.propagate(d, p.K, L, S0, dtype=np.longdouble)
        e_ref = float(np.abs(cov - cld).max() / np.abs(cld).max())
        bound = 1e-13 if w == WEIGHTS[0] else max(1e-13, 4.0 * e_ref)
        for Hm, r in ((None, None), (H, rm)):
            out = nr.run(p, x, u, d, p.K, L, S0, np.zeros((14, 14)), Hm, r)
            e = float(np.abs(out["joint"][:, :, :17, :17] - cov).max() / np.abs(cov).max())
            print("weights %s, m = %d: z block vs cov_reference %.2e (float64 vs longdouble %.2e, bound %.2e)" % (w, 0 if Hm is None else 6, e, e_ref, bound))
            assert e <= bound
            assert not out["joint"][:, :, 17:, :].any() and not out["joint"][:, :, :, 17:].any() and not out["kf"].any()
            ref = cr.report(p, x, u, cov)
            err = np.abs(out["report"] - ref)
            assert np.all(err <= 1e-9 * np.maximum(np.abs(ref), 1.0)), err.max()     # margins divide by s: a few digits of the 1e-13
            assert not out["navrep"][:, :6].any()
            assert np.allclose(out["navrep"][:, 6], ref[:, cr.IDX["SIG_R"]], rtol=1e-9)   # no navigation error: it believes the truth


def test_no_measurement_and_zero_gains_transport_the_navigation_error_open_loop():
    p, par, x, u, s, d = _data()
    S0 = np.stack([cr.handover_s0(x[b, 0])[0] for b in range(2)])
    N0 = 0.25 * S0
    L0 = np.zeros((2, p.K, 3, 17))
    joint, kf, _ = nr.propagate(d, p.K, L0, S0, N0)
    Phi = cr.open_loop_phi(d, p.K)
    want = Phi @ N0 @ np.swapaxes(Phi, 1, 2)
    e = float(np.abs(joint[:, -1, 17:, 17:] - want).max() / np.abs(want).max())
    print("m = 0, zero gains: Xi_K[eps eps] vs Phi N0 Phi' %.2e" % e)
    assert e < 1e-12 and kf.shape == (2, p.K, 14, 0)
    # the truth is not steered, so the estimate's error never reaches it
    assert not joint[:, :, :17, 17:].any()
    assert np.array_equal(joint[:, :, :17, :17], cr.propagate(d, p.K, L0, S0))


@pytest.mark.parametrize("w", WEIGHTS)
def test_float64_against_longdouble_symmetry_and_definiteness(w):
    p, par, x, u, s, d = _data()
    L, _ = tr.gains(d, p.K, *w)
    S0 = np.stack([cr.handover_s0(x[b, 0])[0] for b in range(2)])
    H, rm = pv_model(x[0, 0])
    noise = np.random.default_rng(5).uniform(0.0, 1e-8, 14)
    for Hm, r, nz in ((None, None, None), (H, rm, None), (H, rm, noise), (np.eye(14), np.full(14, 1e-8), noise)):
        j64, k64, cond = nr.propagate(d, p.K, L, S0, 0.25 * S0, Hm, r, nz)
        jld, kld, _ = nr.propagate(d, p.K, L, S0, 0.25 * S0, Hm, r, nz, np.longdouble)
        e = float(np.abs(j64 - jld).max() / np.abs(jld).max())
        ek = float(np.abs(k64 - kld).max()) if k64.size else 0.0
        print("weights %s m = %d w %s: float64 vs longdouble %.2e (gains %.2e), cond(S) %.2e" % (w, k64.shape[-1], nz is not None, e, ek, cond.max()))
        if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps:
            # test_cov_cpu.py allows the n = 17 recursion 1e-12 (K n 2^-52 = 1.9e-13 times the room the stiffer gains need); the joint's
            # dot products are N = 31 long: the same allowance times N / n, times the conditioning of the solve with S
            assert e < 1e-12 * (31.0 / 17.0) * cond.max()
        assert np.array_equal(j64, np.swapaxes(j64, -1, -2))
        lam = np.linalg.eigvalsh(j64)
        print("smallest eigenvalue / max|Xi| %.2e" % (lam.min() / np.abs(j64).max()))
        assert lam.min() >= -1e-12 * np.abs(j64).max()


@pytest.mark.parametrize("b", [0, 1])
def test_monte_carlo_sample_covariance_of_the_joint_within_six_standard_errors(b):
    """N = 8,192 closed loops of the C oracle, each from a Gaussian start (S0 with its factor scaled by 0.1) and fed an estimate whose
    error is sampled by montecarlo.nav_error_samples (N0 = 0.25 S0; r and v measured at every node, 1 sigma 3e-5 of the largest
    component of the start; w = 0: the flyer has no process noise), against the recursion on the joint [z; eps]:
    |S^_ij - Xi_ij| <= 6 sqrt((Xi_ii Xi_jj + Xi_ij^2) / (N - 1)) for EVERY entry of every node."""
    from oracle import dynamics as od
    from successiveconvexification_amd.montecarlo import gaussian_handover, nav_error_samples
    p, par, x, u, s, d = _data()
    N = 8192
    L, _ = tr.gains(d, p.K)
    S0, _ = cr.handover_s0(x[b, 0], scale=0.1)
    N0 = 0.25 * S0
    H, rm = pv_model(x[b, 0])
    sl = slice(b, b + 1)
    out = nr.run(p, x[sl], u[sl], d[sl], p.K, L[sl], S0[None], N0[None], H, rm)
    base = cr.run(p, x[sl], u[sl], d[sl], p.K, L[sl], S0[None])[0]
    dx0 = gaussian_handover(S0, 0, N, 11)
    fed, before = nav_error_samples(d[b], out["kf"][0], H, rm, N0, 0, N, 12)
    xf, uf = nr.chain(od, par, p, cr.rep(x[sl], N), cr.rep(u[sl], N), cr.rep(s[sl], N), cr.rep(L[sl], N), dx0, fed, 10)
    worst, worstK, over = nr.mc_check(xf, uf, before, x[b], u[b], out["joint"][0])
    print("plan %d: worst entry %.2f standard errors (%.2f at node K), %d entries over 6; landing position 1 sigma %.3g without, %.3g with "
          "the navigation term (NAV_R %.3g, EST_R %.3g)" % (b, worst, worstK, over, base[0, cr.IDX["SIG_R"]], out["report"][0, cr.IDX["SIG_R"]],
                                                           out["navrep"][0, nr.NAV_IDX["NAV_R"]], out["navrep"][0, nr.NAV_IDX["EST_R"]]))
    assert over == 0, (worst, over)
    assert out["report"][0, cr.IDX["SIG_R"]] > base[0, cr.IDX["SIG_R"]]


def test_navigation_report_columns():
    p, par, x, u, s, d = _data()
    L, _ = tr.gains(d, p.K)
    S0 = np.stack([cr.handover_s0(x[b, 0])[0] for b in range(2)])
    H, rm = pv_model(x[0, 0])
    out = nr.run(p, x, u, d, p.K, L, S0, 0.25 * S0, H, rm)
    blind = nr.run(p, x, u, d, p.K, L, S0, 0.25 * S0)
    j, nv = out["joint"], out["navrep"]
    for b in range(2):
        P = j[b, -1, 17:, 17:]
        assert nv[b, nr.NAV_IDX["NAV_R"]] == np.sqrt(np.trace(P[1:4, 1:4])) and nv[b, nr.NAV_IDX["NAV_Q"]] == np.sqrt(np.trace(P[7:11, 7:11]))
        assert nv[b, nr.NAV_IDX["NAV_PEAK"]] >= np.sqrt(np.trace(0.25 * S0[b])) * (1 - 1e-15)
        E = j[b, -1, :14, :14] - j[b, -1, :14, 17:] - j[b, -1, 17:, :14] + P
        assert abs(nv[b, nr.NAV_IDX["EST_V"]] - np.sqrt(np.trace(E[4:7, 4:7]))) <= 1e-15
        assert np.array_equal(out["navsig"][b, :, 2], np.sqrt(j[b, :, 19, 19])) and np.array_equal(out["sig"][b, :, 2], np.sqrt(j[b, :, 2, 2]))
    print("NAV_R measured %s, inertial only %s; SIG_R measured %s, inertial only %s" % (nv[:, 1], blind["navrep"][:, 1],
                                                                                    out["report"][:, 1], blind["report"][:, 1]))
    # measurements shrink the navigation error and with it the landing dispersion
    assert np.all(nv[:, :6] <= blind["navrep"][:, :6]) and np.all(out["report"][:, 1] < blind["report"][:, 1])
    # a NaN in one trajectory's N0 poisons both of its reports, and only them
    N0 = 0.25 * S0
    N0[1, 3, 3] = np.nan
    bad = nr.run(p, x, u, d, p.K, L, S0, N0, H, rm)
    assert np.isnan(bad["report"][1]).all() and np.isnan(bad["navrep"][1]).all()
    assert np.array_equal(bad["report"][0], out["report"][0]) and np.array_equal(bad["navrep"][0], nv[0])


def test_header_binding_and_julia_carry_the_same_symbols():
    from successiveconvexification_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "scvx.h")).read()
    jl = open(os.path.join(ROOT, "julia", "ScvxAMD.jl")).read()
    nargs = {"scvx_nav_cov_f64": 19, "scvx_nav_cov_f64_host": 19, "scvx_track_fly_nav_f64": 14, "scvx_track_fly_nav_f64_host": 14,
             "scvx_batch_nav_cov": 16, "scvx_batch_track_fly_nav": 11}
    for sym, n in nargs.items():
        m = re.search(r"\bint %s\(([^;]*?)\);" % sym, hdr, flags=re.S)
        assert m, sym
        assert len(m.group(1).split(",")) == n, sym
        assert len(_lib.SIGNATURES[sym][1]) == n, sym
        j = re.search(r"ccall\(\(:%s, LIB\), Cint,\s*\(([^)]*)\)" % sym, jl, flags=re.S)
        assert j, sym
        assert len([a for a in j.group(1).split(",") if a.strip()]) == n, sym
    # the old call keeps its argument list: the navigation input is a call of its own
    assert len(_lib.SIGNATURES["scvx_track_fly_f64"][1]) == 13 and len(_lib.SIGNATURES["scvx_cov_propagate_f64"][1]) == 13
    mac = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define SCVX_NAV_([A-Z_]+) (\d+)", hdr)}
    assert mac.pop("NREP") == 8 == _lib.NAV_NREP == nr.NAV_NREP
    strip = lambda n: n[4:] if n.startswith("NAV_") else n   # noqa: E731   SCVX_NAV_M, SCVX_NAV_EST_R: NAV_M, EST_R
    assert mac == {strip(n): i for n, i in _lib.NAV_INDEX.items()} and _lib.NAV_COLUMNS == nr.NAV_COLUMNS
    for name, i in _lib.NAV_INDEX.items():
        assert int(re.search(r"const NAV_%s = (\d+)" % strip(name), jl).group(1)) == i
    assert int(re.search(r"#define SCVX_ABI_VERSION (\d+)", hdr).group(1)) == 4 == _lib.ABI_VERSION
    # outside install!(): that function's body is pinned to the reference's by test_abi_harness.py
    assert jl.index("function navigation(b::Batch") < jl.index("function install!")
    assert "navigation" not in jl[jl.index("function install!"):]
    # the header states the model and its limits
    for word in ("Joseph", "FIRST ORDER", "no measurement at node K", "the clamp is not modelled", "norm direction"):
        assert word in hdr, word


def test_nav_report_and_argument_helpers():
    from successiveconvexification_amd import _lib
    from successiveconvexification_amd._calls import NAV_DENSE, dense_names
    from successiveconvexification_amd.dynamics import CovReport, NavReport, _nav_model
    from successiveconvexification_amd.montecarlo import dispersion_summary
    raw = np.arange(3 * 16, dtype=float).reshape(3, 16)
    nav = 100.0 + np.arange(3 * 8, dtype=float).reshape(3, 8)
    r = NavReport(raw, nav, navsig=np.zeros((3, 4, 14)), kf=np.zeros((3, 3, 14, 6)))
    assert isinstance(r, CovReport) and len(r) == 3 and r.sig is None and r.joint is None and r.covK is None and r.cov is None
    for n, i in _lib.COV_INDEX.items():
        assert np.array_equal(getattr(r, n), raw[:, i])
    for n, i in _lib.NAV_INDEX.items():
        assert np.array_equal(getattr(r, n), nav[:, i])
    assert r.tightest()[0] == raw[0, _lib.COV_INDEX["N_MASS"]]
    assert dispersion_summary(r, np.zeros(3, int))["stats"]["SIG_R"]["max"] == raw[2, 1]      # read as it is
    assert _nav_model(None, None) == (0, None, None) and _nav_model(np.zeros((0, 14)), None) == (0, None, None)
    m, H, rm = _nav_model(np.eye(14)[1:4], 2.0)
    assert m == 3 and H.flags.c_contiguous and rm.tolist() == [2.0] * 3
    for bad in ((np.eye(3), 1.0), (np.eye(14)[1:4], np.ones(2)), (np.eye(14)[1:4], None)):
        with pytest.raises(ValueError):
            _nav_model(*bad)
    assert dense_names(True, NAV_DENSE) == {"sig", "navsig", "kf", "joint"} and dense_names(False, NAV_DENSE) == set()
    assert dense_names("kf", NAV_DENSE) == {"kf"}
    with pytest.raises(ValueError):
        dense_names(["cov"], NAV_DENSE)


def test_measurement_rows_and_nav_error_samples():
    from successiveconvexification_amd.montecarlo import measurement_rows, nav_error_samples
    assert np.array_equal(measurement_rows("r"), np.eye(14)[1:4]) and np.array_equal(measurement_rows(["v", "r"]), np.eye(14)[1:7])
    assert np.array_equal(measurement_rows("rvqw"), np.eye(14)[1:]) and measurement_rows("").shape == (0, 14)
    for bad in ("m", "rr", ["x"]):
        with pytest.raises(ValueError):
            measurement_rows(bad)
    p, par, x, u, s, d = _data()
    L, _ = tr.gains(d, p.K)
    S0, _ = cr.handover_s0(x[0, 0], scale=0.1)
    N0 = 0.25 * S0
    H, rm = pv_model(x[0, 0])
    joint, kf, _ = nr.propagate(d[:1], p.K, L[:1], S0[None], N0[None], H, rm)
    fed, before = nav_error_samples(d[0], kf[0], H, rm, N0, 0, 12, 99)
    assert fed.shape == (12, p.K, 14) and before.shape == (12, p.K + 1, 14)
    f2, b2 = nav_error_samples(d[0], kf[0], H, rm, N0, 5, 9, 99)
    assert np.array_equal(f2, fed[5:9]) and np.array_equal(b2, before[5:9])              # shards agree with the whole batch
    assert not np.array_equal(fed, nav_error_samples(d[0], kf[0], H, rm, N0, 0, 12, 100)[0])
    A = tr.split_tiles(d[:1], p.K)[0][0]
    want = np.einsum("kij,bkj->bki", A, fed)                                             # eps_{k+1} = A_k eps+_k: no process noise
    assert np.abs(before[:, 1:] - want).max() <= 14 * 2.0 ** -52 * np.abs(want).max()    # 14-term sums in another order
    # without a measurement the estimate is never corrected
    f0, b0 = nav_error_samples(d[0], None, None, None, N0, 0, 4, 99)
    assert np.array_equal(f0, b0[:, :-1]) and np.array_equal(b0[:, 0], before[:4, 0])
    # the samples' own covariance is the recursion's eps block (the truth plays no part in it): six standard errors, every entry
    N = 4096
    fed, before = nav_error_samples(d[0], kf[0], H, rm, N0, 0, N, 3)
    z = before - before.mean(axis=0)
    Sh = np.einsum("bki,bkj->kij", z, z) / (N - 1)
    P = joint[0, :, 17:, 17:]
    dg = np.diagonal(P, axis1=1, axis2=2)
    se = np.sqrt((dg[:, :, None] * dg[:, None, :] + P ** 2) / (N - 1))
    print("nav_error_samples: worst entry %.2f standard errors" % np.max(np.abs(Sh - P)[se > 0] / se[se > 0]))
    assert np.all(np.abs(Sh - P) <= 6.0 * se)
