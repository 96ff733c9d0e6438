"""Flight check without a GPU: the independent reference (tests/flight_reference.py) against closed forms and the C oracle, the three
bindings (header, _lib.SIGNATURES, julia/ScvxAMD.jl) against each other, montecarlo.flight_summary, and the committed fixture."""
import os
import re

import numpy as np
import pytest

import flight_reference as fr
from conftest import GOLDEN, ROOT, random_segments


def _po():
    from oracle import model
    return model.base_prob_scaled()


@pytest.mark.parametrize("nsub", [1, 4, 10])
def test_substep_chain_reproduces_the_oracles_whole_segments(nsub):
    """nsub one-substep segments with the hold interpolated to the substep boundaries = od.propagate(..., nsub), to rounding."""
    from oracle import dynamics as od
    p = _po()
    x, u, sigma = random_segments(p, 6, 50, 20261016)
    par = od.Params(p)
    _, _, xfly = fr.chain(od, par, x, u, sigma, nsub, fr.PLAN)
    e = od.propagate(par, x, u, sigma, 1.0 / 51, nsub)
    assert np.abs(xfly[:, 1:] - e).max() < 1e-15
    assert np.array_equal(xfly[:, 0], x[:, 0])
    # PLAN GAP is the largest whole-segment defect
    r, _ = fr.fly(od, p, x, u, sigma, nsub, fr.PLAN, par)
    assert np.abs(r[:, fr.IDX["GAP"]] - np.abs(x[:, 1:] - e).max(axis=(1, 2))).max() < 1e-15


def test_shoot_chain_is_the_composition_of_segments():
    """SHOOT: the end of segment k starts segment k + 1 -- composed by hand from od.propagate on two-node plans."""
    from oracle import dynamics as od
    p = _po()
    x, u, sigma = random_segments(p, 3, 6, 5)
    par = od.Params(p)
    _, _, xfly = fr.chain(od, par, x, u, sigma, 4, fr.SHOOT)
    cur = x[:, 0]
    for k in range(6):
        xx = np.stack([cur, cur], axis=1)
        cur = od.propagate(par, xx, u[:, k:k + 2], sigma, 1.0 / 7, 4)[:, 0]
        assert np.abs(xfly[:, k + 1] - cur).max() < 1e-15


def test_tmin_dip_between_two_nodes_on_the_bound_is_the_chord_minimum():
    """Two nodes at |u| = Tmin with different directions: the hold is a chord of the sphere, so G_TMIN is Tmin minus the smallest
    chord norm at the substep boundaries -- closed form; every node sits on the bound (node-wise G_TMIN = 0)."""
    from oracle import dynamics as od
    p = _po()
    K, nsub = p.K, 10
    x, u, sigma = random_segments(p, 1, K, 3)
    ang = np.radians(15.0)
    a, b = np.array([1.0, 0.0, 0.0]), np.array([np.cos(ang), np.sin(ang), 0.0])
    u[0, :] = p.Tmin * a
    u[0, 1::2] = p.Tmin * b
    r, _ = fr.fly(od, p, x, u, sigma, nsub, fr.SHOOT)
    lam = np.arange(nsub + 1) / nsub
    # |(1 - l) a + l b|^2 = 1 - 2 l (1 - l) (1 - cos ang) for unit a, b
    chord = p.Tmin * np.sqrt(1.0 - 2.0 * lam * (1.0 - lam) * (1.0 - np.cos(ang)))
    want = p.Tmin - chord.min()
    assert want > 1e-3 * p.Tmin
    assert abs(r[0, fr.IDX["G_TMIN"]] - want) < 1e-15
    assert abs(want - p.Tmin * (1.0 - np.cos(ang / 2))) < 1e-15       # the midpoint is a sample at even nsub
    assert np.abs(p.Tmin - np.linalg.norm(u[0], axis=-1)).max() < 1e-15
    # the control rows are convex / linear in the hold: never above their node values
    assert r[0, fr.IDX["G_TMAX"]] <= (np.linalg.norm(u[0], axis=-1) - p.Tmax).max() + 1e-15


def test_report_columns_by_hand_and_nan_rows():
    from oracle import dynamics as od
    from dataclasses import replace
    p = replace(_po(), enforce_dp=True, dpMax=0.02)
    x, u, sigma = random_segments(p, 3, 8, 11)
    p = replace(p, K=8)
    S, US, xfly = fr.chain(od, od.Params(p), x, u, sigma, 2, fr.SHOOT)
    r = fr.report(p, x, S, US, xfly)
    assert np.all(np.isneginf(r[:, fr.IDX["G_FIN"]])) and np.all(np.isfinite(r[:, fr.IDX["G_DP"]]))
    t = 1
    s = S[t].reshape(-1, 14)
    assert r[t, fr.IDX["G_DP"]] == (np.linalg.norm(s[:, 4:7], axis=1) - np.sqrt(2 * p.dpMax / p.rho)).max()
    assert r[t, fr.IDX["G_GLIDE"]] == (np.tan(np.radians(p.gammaGs)) * np.hypot(s[:, 2], s[:, 3]) - s[:, 1]).max()
    assert r[t, fr.IDX["MASS_END"]] == xfly[t, -1, 0] and r[t, fr.IDX["MISS_R"]] == np.linalg.norm(xfly[t, -1, 1:4] - p.rIf)
    x2 = x.copy()
    x2[2, 0, 5] = np.nan
    r2, _ = fr.fly(od, p, x2, u, sigma, 2, fr.SHOOT)
    assert np.array_equal(r2[:2], r[:2])
    assert all(np.isnan(r2[2, fr.IDX[n]]) for n in fr.STATE_COLUMNS)
    assert all(np.isfinite(r2[2, fr.IDX[n]]) for n in ("G_TMAX", "G_TMIN", "G_GIMBAL"))


def _header_macros():
    hdr = open(os.path.join(ROOT, "include", "scvx.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define SCVX_FLIGHT_([A-Z_]+) (\d+)", hdr)}


def test_header_binding_and_julia_carry_the_same_symbols_and_indices():
    from successiveconvexification_amd import _lib
    mac = _header_macros()
    assert mac.pop("SHOOT") == _lib.FLIGHT_SHOOT == fr.SHOOT == 0 and mac.pop("PLAN") == _lib.FLIGHT_PLAN == fr.PLAN == 1
    assert mac.pop("NREP") == _lib.FLIGHT_NREP == fr.NREP == 16
    assert mac == _lib.FLIGHT_INDEX == fr.IDX and len(mac) == 16
    assert _lib.FLIGHT_COLUMNS == fr.COLUMNS
    hdr = open(os.path.join(ROOT, "include", "scvx.h")).read()
    jl = open(os.path.join(ROOT, "julia", "ScvxAMD.jl")).read()
    for sym in ("scvx_flight_check_f64", "scvx_flight_check_f64_host", "scvx_batch_flight_check"):
        assert re.search(r"\bint %s\(" % sym, hdr), sym
        assert sym in _lib.SIGNATURES, sym
        assert re.search(r"ccall\(\(:%s, LIB\)" % sym, jl), sym
    # argument counts: ctx, B, K, x, u, sigma, nsub, mode, report, xfly / batch, nsub, mode, report, xfly
    assert len(_lib.SIGNATURES["scvx_flight_check_f64"][1]) == len(_lib.SIGNATURES["scvx_flight_check_f64_host"][1]) == 10
    assert len(_lib.SIGNATURES["scvx_batch_flight_check"][1]) == 5
    jmac = {m.group(1): int(m.group(2)) for m in re.finditer(r"const FLIGHT_([A-Z_]+) = (\d+)", jl)}
    assert jmac == _header_macros()
    assert "function flight_check(b::Batch; nsub" in jl


def test_flight_report_views_and_ok():
    from successiveconvexification_amd import _lib
    from successiveconvexification_amd.dynamics import FlightReport
    raw = np.full((3, 16), -1.0)
    raw[:, _lib.FLIGHT_INDEX["G_DP"]] = -np.inf
    raw[:, _lib.FLIGHT_INDEX["G_FIN"]] = -np.inf
    raw[1, _lib.FLIGHT_INDEX["G_TMIN"]] = 2e-4
    raw[2, _lib.FLIGHT_INDEX["G_RATE"]] = np.nan
    r = FlightReport(raw)
    assert len(r) == 3 and r.G_TMIN[1] == 2e-4 and r.raw is not None and r.xfly is None
    assert np.shares_memory(r.G_TMIN, r.raw)
    assert r.active() == ("G_MASS", "G_GLIDE", "G_TILT", "G_RATE", "G_TMAX", "G_TMIN", "G_GIMBAL")
    assert r.ok(0.0).tolist() == [True, False, False] and r.ok(1e-3).tolist() == [True, True, False]


def test_flight_summary_on_a_synthetic_report():
    from successiveconvexification_amd import _lib
    from successiveconvexification_amd.montecarlo import flight_summary
    I = _lib.FLIGHT_INDEX
    N = 200
    rng = np.random.default_rng(0)
    raw = np.full((N, 16), -0.5)
    raw[:, I["GAP"]] = rng.uniform(1e-9, 1e-7, N)
    raw[:, I["MASS_END"]] = 0.6
    raw[:, I["G_DP"]] = -np.inf
    raw[:, I["G_FIN"]] = -np.inf
    raw[:, I["G_TMIN"]] = np.linspace(-1e-4, 1e-4, N)
    status = np.zeros(N, np.int32)
    status[:20] = 1
    status[20:25] = 3
    s = flight_summary(raw, status, tol=0.0)
    assert s["n"] == N and s["counts"]["converged"] == 175 == s["converged"] and s["counts"]["running"] == 20 and s["counts"]["solver"] == 5
    assert sum(s["counts"].values()) == N
    conv = raw[status == 0]
    assert s["feasible_share"] == pytest.approx(np.mean(conv[:, I["G_TMIN"]] <= 0.0))
    assert s["stats"]["GAP"]["max"] == conv[:, I["GAP"]].max() and s["stats"]["GAP"]["median"] == np.median(conv[:, I["GAP"]])
    assert s["stats"]["G_TMIN"]["p99"] == np.percentile(conv[:, I["G_TMIN"]], 99)
    assert s["stats"]["G_DP"]["max"] == -np.inf and s["stats"]["MASS_END"]["min"] == 0.6
    assert flight_summary(raw, status, tol=1e-3)["feasible_share"] == 1.0
    # a report gathered over ranks: [world][B][16] flattens to the same thing; no converged plan: no statistics
    assert flight_summary(raw.reshape(4, 50, 16), status, 0.0) == s
    none = flight_summary(raw, np.ones(N, np.int32))
    assert none["converged"] == 0 and none["feasible_share"] is None and none["stats"]["GAP"] is None
    with pytest.raises(ValueError):
        flight_summary(raw, status[:-1])


def test_fixture_reports_are_rederived_by_the_reference():
    """tests/golden/oracle_flight_runs.npz (make_oracle_flight_runs.py): two plans the oracle converges on; the stored reports follow
    from the stored plans, and they show what only the flight check shows -- the thrust bound held at the nodes and violated in between."""
    from dataclasses import replace
    from oracle import dynamics as od, model
    g = np.load(os.path.join(GOLDEN, "oracle_flight_runs.npz"))
    p = replace(model.base_prob_scaled(), mdry=0.55, nuTol=1e-6, delTol=1e-3, imax=40, tf_guess=8.0)
    x, u, sigma, nsub = g["x"], g["u"], g["sigma"], int(g["nsub"])
    assert x.shape == (2, p.K + 1, 14) and nsub == 10
    for name, mode, n in (("report_shoot", fr.SHOOT, nsub), ("report_plan", fr.PLAN, nsub), ("report_shoot_nsub40", fr.SHOOT, 40)):
        r, _ = fr.fly(od, p, x, u, sigma, n, mode)
        assert np.array_equal(r, g[name]), name
    rs, rp = g["report_shoot"], g["report_plan"]
    assert np.all(rs[:, fr.IDX["G_TMIN"]] > 1e-4) and np.all(rp[:, fr.IDX["G_TMIN"]] > 1e-4)
    assert (p.Tmin - np.linalg.norm(u, axis=-1)).max() <= 1e-8
    assert np.all(rs[:, fr.IDX["GAP"]] < 1e-6) and np.all(rp[:, fr.IDX["GAP"]] < 1e-6)
    assert np.abs(g["report_shoot_nsub40"][:, 0] - rs[:, 0]).max() < 1e-7
    # the chain is benign on these plans: measured sensitivity of a few units
    for eps in (1e-12, 1e-9, 1e-6):
        A = fr.sensitivity(od, p, x, u, sigma, nsub, eps)
        assert 1.0 <= A < 10.0, (eps, A)
