"""Order statistics and per-node back-offs of the sampled dispersion without a GPU: the bindings of the eight new calls (header,
_lib.SIGNATURES, julia/ScvxAMD.jl) against each other, montecarlo.quantile_ranks against numpy, the reference's per-node values
(tests/mc_quantile_reference.py on mc_reference.chain), montecarlo.margins_from_quantiles on hand-made order statistics, and the
statistical anchor: the per-node quantiles of 8,192 flights through the C oracle against the first-order s(k) of tests/cov_reference.py.

Data: the two plans the oracle converges on (tests/golden/oracle_flight_runs.npz), tiles from oracle.dynamics.linearize."""
import os
import re
from statistics import NormalDist

import numpy as np
import pytest

import cov_reference as cr
import margin_reference as mgr
import mc_quantile_reference as qr
import mc_reference as mr
import track_reference as tr
from conftest import ROOT
from test_cov_cpu import _data

Q_SAMPLES = 8192
Q_SEED = 20261019

NEW = {"scvx_order_stats_f64": 9, "scvx_order_stats_f64_host": 9, "scvx_track_mc_q_f64": 27, "scvx_track_mc_q_f64_host": 27,
       "scvx_track_mc_nav_q_f64": 39, "scvx_track_mc_nav_q_f64_host": 39, "scvx_batch_track_mc_q": 24, "scvx_batch_track_mc_nav_q": 35}
OLD = {"scvx_track_mc_f64": 22, "scvx_track_mc_f64_host": 22, "scvx_batch_track_mc": 19, "scvx_track_mc_nav_f64": 34,
       "scvx_track_mc_nav_f64_host": 34, "scvx_batch_track_mc_nav": 30}


def test_header_binding_and_julia_carry_the_eight_symbols():
    from successiveconvexification_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "scvx.h")).read()
    jl = open(os.path.join(ROOT, "julia", "ScvxAMD.jl")).read()
    for sym, n in {**NEW, **OLD}.items():
        m = re.search(r"\bint %s\(([^;]*?)\);" % sym, hdr, flags=re.S)
        assert m, sym
        assert len(m.group(1).split(",")) == n, sym
        assert len(_lib.SIGNATURES[sym][1]) == n, sym
        j = re.search(r"ccall\(\(:%s, LIB\), Cint,\s*\(([^)]*)\)" % sym, jl, flags=re.S)
        assert j, sym
        assert len([a for a in j.group(1).split(",") if a.strip()]) == n, sym
    # each _q form is the argument list of the call it extends, verbatim, then the five new ones
    tail = r"int nq,\s*const int \*ranks,\s*double \*flightq(_dev)?,\s*double \*pathq(_dev)?,\s*double \*pathv(_dev)?$"
    for new, old in (("scvx_track_mc_q_f64", "scvx_track_mc_f64"), ("scvx_track_mc_q_f64_host", "scvx_track_mc_f64_host"),
                     ("scvx_track_mc_nav_q_f64", "scvx_track_mc_nav_f64"), ("scvx_track_mc_nav_q_f64_host", "scvx_track_mc_nav_f64_host"),
                     ("scvx_batch_track_mc_q", "scvx_batch_track_mc"), ("scvx_batch_track_mc_nav_q", "scvx_batch_track_mc_nav")):
        norm = lambda s: re.sub(r"\s+", " ", re.search(r"\bint %s\(([^;]*?)\);" % s, hdr, flags=re.S).group(1)).strip()   # noqa: E731
        a, b = norm(new), norm(old)
        assert a.startswith(b + ", "), new
        assert re.search(tail, a[len(b) + 2:]), (new, a[len(b) + 2:])
        assert _lib.SIGNATURES[new][1][:len(_lib.SIGNATURES[old][1])] == _lib.SIGNATURES[old][1], new
    assert int(re.search(r"#define SCVX_ABI_VERSION (\d+)", hdr).group(1)) == 4 == _lib.ABI_VERSION
    assert int(re.search(r"#define SCVX_Q_MAX (\d+)", hdr).group(1)) == 16 == int(re.search(r"const Q_MAX = (\d+)", jl).group(1))
    assert "const void *reserved" in re.search(r"\bint scvx_track_mc_q_f64\(([^;]*?)\);", hdr, flags=re.S).group(1)
    # outside install!(): that function's body is pinned to the reference's by test_abi_harness.py
    assert jl.index("function track_mc_q(b::Batch") < jl.index("function install!")
    assert "order_stats" not in jl[jl.index("function install!"):]
    # the limits the header has to state, and the sentence it no longer carries
    for phrase in ("inverted_cdf", "SELECTION", "267 MB", "before the clamp", "standard error", "shared across plans", "tan(gammaGs) times"):
        assert phrase.lower() in hdr.lower(), phrase
    assert "take them from `flights`" not in hdr


@pytest.mark.parametrize("S", [1, 2, 7, 64, 1000])
def test_quantile_ranks_against_numpy(S):
    from successiveconvexification_amd.montecarlo import quantile_ranks
    probs = [0.0, 1e-9, 0.5, 0.99865, 1.0]
    rk = quantile_ranks(probs, S)
    assert rk.dtype == np.int32 and rk.shape == (5,) and np.array_equal(rk, qr.ranks(probs, S))
    assert rk[0] == 0 and rk[-1] == S - 1 and np.all(np.diff(rk) >= 0)
    rng = np.random.default_rng(S)
    for _ in range(20):
        a = rng.standard_normal(S)
        srt = np.sort(a)
        for q, r in zip(probs, rk):
            assert srt[r] == np.quantile(a, q, method="inverted_cdf"), (S, q, r)
    assert np.array_equal(quantile_ranks(0.5, S), qr.ranks([0.5], S))
    with pytest.raises(ValueError):
        quantile_ranks([1.5], S)
    with pytest.raises(ValueError):
        quantile_ranks([0.5], 0)


def test_reference_order_stats_and_per_node_values():
    """NaNs sort last and +-0 compare equal; the per-node values are functions of mc_reference.chain's xfly and cmd alone"""
    from oracle import dynamics as od
    v = np.array([[3.0, -np.inf, np.nan, -0.0, 0.0, np.inf, -5e-324, 2.0]])
    o = qr.order_stats(v, [0, 1, 2, 3, 4, 5, 6, 7])
    assert o[0, 0] == -np.inf and o[0, 1] == -5e-324 and o[0, 2] == 0.0 and o[0, 3] == 0.0 and o[0, 6] == np.inf and np.isnan(o[0, 7])
    assert abs(qr.quantile_se(0.5, 8192) - np.sqrt(0.25 / 8192) * np.sqrt(2 * np.pi)) < 1e-15
    p, par, x, u, s, d = _data()
    L, _ = tr.gains(d, p.K)
    rng = np.random.default_rng(1)
    N = 6
    dx0 = np.zeros((N, 14))
    dx0[:, 1:7] = 1e-3 * rng.standard_normal((N, 6))
    imp = np.zeros((N, p.K, 14))
    imp[:, 4, 0] = 1e-3                                                # the mass after segment 4: node 5 sees it
    for flags in (0, tr.CLAMP):
        S_, US, xf, uf, cmd = mr.chain(od, par, p, cr.rep(x[:1], N), cr.rep(u[:1], N), cr.rep(s[:1], N), cr.rep(L[:1], N), dx0, 2, flags, imp)
        v = qr.path_values(p, xf, cmd, u[0, 0])
        assert v.shape == (N, p.K + 1, 5)
        assert np.array_equal(v[:, :, 0], xf[:, :, 0]) and np.array_equal(v[:, 5, 0], S_[:, 4, -1, 0] + 1e-3)
        assert np.array_equal(v[:, 0, 0], np.full(N, x[0, 0, 0])) and np.all(v[:, 0, 4] == np.linalg.norm(u[0, 0, :3]))
        assert np.array_equal(v[:, 1:, 4], cmd)
        if flags == 0:                                                 # without the clamp the command is what is applied
            assert np.allclose(v[:, 1:, 4], np.linalg.norm(uf[:, 1:, :3], axis=-1), rtol=4 * qr.EPS, atol=0)
        assert np.allclose(v[:, :, 3], np.linalg.norm(xf[:, :, 11:14], axis=-1), rtol=4 * qr.EPS, atol=0)
    g = qr.plan_values(p, x[0], u[0])
    assert g.shape == (p.K + 1, 5) and np.array_equal(g[:, 0], x[0, :, 0])
    assert np.allclose(g[:, 4], np.linalg.norm(u[0, :, :3], axis=-1), rtol=4 * qr.EPS, atol=0)


def _hand_made(p, B=3, seed=0):
    rng = np.random.default_rng(seed)
    K1 = p.K + 1
    x = rng.standard_normal((B, K1, 14)) * 0.1
    x[:, :, 0] = rng.uniform(p.mdry, p.mwet, (B, K1))
    x[:, :, 1] = np.linspace(0.5, 0.0, K1)[None] + 1e-4           # the height: the glide width moves along the plan
    u = rng.standard_normal((B, K1, 3))
    return x, u


def test_margins_from_quantiles_formulas_caps_and_zeros():
    from successiveconvexification_amd import montecarlo as mc
    p, *_ = _data()
    B, K1, K = 3, p.K + 1, p.K
    x, u = _hand_made(p, B)
    g = np.stack([qr.plan_values(p, x[b], u[b]) for b in range(B)])
    assert np.allclose(mc.path_functions(p, x, u), g, rtol=1e-15, atol=0)
    g = mc.path_functions(p, x, u)
    cap = 0.25
    tg = np.tan(np.deg2rad(p.gammaGs))
    sqcm = np.sqrt((1.0 - np.cos(np.deg2rad(p.thetaMax))) / 2.0)
    width = {"THRUST": p.Tmax - p.Tmin, "MASS": p.mwet - p.mdry, "TILT": sqcm, "RATE": p.omMax}
    small = 1e-3
    qlo, qhi = g - small, g + small * np.array([1.0, 20.0, 3.0, 4.0, 5.0])
    lo, hi, pm = mc.margins_from_quantiles(p, x, u, qlo, qhi, "all", cap)
    # the formulas, below every cap: lo = |u| - Q_{1-p}(T), hi = Q_p(T) - |u| -- an ASYMMETRIC pair --, mass = mbar - Q_{1-p}(m), ...
    assert np.array_equal(lo, g[:, :, 4] - qlo[:, :, 4]) and np.array_equal(hi, qhi[:, :, 4] - g[:, :, 4]) and not np.array_equal(lo, hi)
    assert np.array_equal(pm[:, 1:, 0], (g[:, :, 0] - qlo[:, :, 0])[:, 1:])
    gw = cap * np.maximum(x[:, :, 1], 0.0) / tg
    ref_gl = np.minimum(qhi[:, :, 1] - g[:, :, 1], cap * (np.maximum(x[:, :, 1], 0.0) * (1.0 / tg)))
    assert np.array_equal(pm[:, 1:K, 1], ref_gl[:, 1:K])
    assert np.any(pm[:, 1:K, 1] < 20 * small * 0.999) and np.any(pm[:, 1:K, 1] == qhi[:, 1:K, 1] - g[:, 1:K, 1])   # the moving width caps the late nodes only
    assert np.all(pm[:, 1:K, 1] <= gw[:, 1:K] * (1 + 4 * qr.EPS))
    assert np.array_equal(pm[:, :K, 2], (qhi[:, :, 2] - g[:, :, 2])[:, :K]) and np.array_equal(pm[:, 1:K, 3], (qhi[:, :, 3] - g[:, :, 3])[:, 1:K])
    # every forced zero: glide / tilt / rate at node K, mass / glide / rate at node 0 -- tilt at node 0 and mass at node K are live
    assert not pm[:, K, 1:].any() and not pm[:, 0, [0, 1, 3]].any() and pm[:, 0, 2].all() and pm[:, K, 0].all()
    # a quantile on the wrong side of the plan's own value: the back-off is 0, never negative
    l2, h2, pm2 = mc.margins_from_quantiles(p, x, u, g + small, g - small, "all", cap)
    assert not l2.any() and not h2.any() and not pm2.any()
    # the caps: cap times the constant widths
    big = 1e3
    l3, h3, pm3 = mc.margins_from_quantiles(p, x, u, g - big, g + big, "all", cap)
    assert np.all(l3 == cap * width["THRUST"]) and np.all(h3 == cap * width["THRUST"])
    assert np.all(pm3[:, 1:, 0] == cap * width["MASS"]) and np.all(pm3[:, :K, 2] == cap * width["TILT"])
    assert np.all(pm3[:, 1:K, 3] == cap * width["RATE"])
    assert np.array_equal(pm3[:, 1:K, 1], (cap * (np.maximum(x[:, :, 1], 0.0) * (1.0 / tg)))[:, 1:K])
    xn = x.copy()
    xn[:, 7, 1] = -0.5                                                # below the pad: the width is 0, not negative
    assert not mc.margins_from_quantiles(p, xn, u, g - big, g + big, ("glide",), cap)[2][:, 7, 1].any()
    # NaN -> zeros for that trajectory only, in the selected kinds only
    qn = qhi.copy()
    qn[1, 9, 3] = np.nan                                               # RATE of trajectory 1
    l4, h4, pm4 = mc.margins_from_quantiles(p, x, u, qlo, qn, "all", cap)
    assert not l4[1].any() and not h4[1].any() and not pm4[1].any()
    assert np.array_equal(l4[[0, 2]], lo[[0, 2]]) and np.array_equal(pm4[[0, 2]], pm[[0, 2]])
    l5, h5, pm5 = mc.margins_from_quantiles(p, x, u, qlo, qn, ("thrust", "mass"), cap)
    assert np.array_equal(l5, lo) and np.array_equal(pm5[:, :, 0], pm[:, :, 0])                 # RATE is not selected: its NaN is not read
    # unselected kinds untouched: they keep the values of `current`, zeros without it
    cur = (np.full((B, K1), 0.11), np.full((B, K1), 0.12), np.full((B, K1, 4), 0.13))
    l6, h6, pm6 = mc.margins_from_quantiles(p, x, u, qlo, qhi, ("tilt",), cap, current=cur)
    assert np.all(l6 == 0.11) and np.all(h6 == 0.12) and np.all(pm6[:, :, [0, 1, 3]] == 0.13) and np.array_equal(pm6[:, :, 2], pm[:, :, 2])
    assert np.all(cur[2] == 0.13)                                      # the caller's arrays are not written
    l7, h7, pm7 = mc.margins_from_quantiles(p, x, u, qlo, qhi, ("thrust",), cap)
    assert np.array_equal(l7, lo) and not pm7.any()
    for bad in ((), ("thrust", "fins"), "thrust"):
        with pytest.raises(ValueError):
            mc.margins_from_quantiles(p, x, u, qlo, qhi, bad, cap)
    with pytest.raises(ValueError):
        mc.margins_from_quantiles(p, x, u, qlo[:, :, :4], qhi, "all", cap)


def test_report_carries_the_quantiles_by_name():
    from successiveconvexification_amd import _lib
    from successiveconvexification_amd.dynamics import McNavReport, McReport, _McQ
    mq = _McQ([0.5, 0.99], True, ("flights", "pathv"))
    assert mq.on and set(mq.rest) == {"flights"} and mq.want_pv
    f = mq.fields(2, 3, 70)
    assert list(f) == ["nq", "ranks", "flightq", "pathq", "pathv"]
    assert f["nq"] == 2 and mq.ranks.tolist() == [34, 69] and mq.flightq.shape == (2, 16, 2) and mq.pathq.shape == (2, 4, 5, 2)
    assert mq.pathv.shape == (2, 4, 5, 70) and f["ranks"] is mq.ranks and f["flightq"] is mq.flightq and f["pathq"] is mq.pathq
    assert f["pathv"] is mq.pathv
    mq.flightq[:] = np.arange(64.0).reshape(2, 16, 2)
    mq.pathq[:] = np.arange(80.0).reshape(2, 4, 5, 2)
    rep = McReport(np.zeros((2, 48)), None, None)._with_q(mq)
    assert np.array_equal(rep.quantile("MISS_R", 0.99), mq.flightq[:, _lib.FLIGHT_INDEX["MISS_R"], 1])
    assert np.array_equal(rep.path_quantile("THRUST", 0.5), mq.pathq[:, :, 4, 0]) and rep.pathv is mq.pathv and rep.probs.tolist() == [0.5, 0.99]
    with pytest.raises(ValueError):
        rep.quantile("MISS_R", 0.9)
    off = _McQ(None, False, True)
    assert not off.on and off.rest is True
    plain = McReport(np.zeros((2, 48)), None, None)._with_q(off)
    assert plain.q is None and plain.pathq is None and plain.pathv is None and plain.ranks is None
    with pytest.raises(ValueError):
        plain.quantile("MISS_R", 0.5)
    lean = _McQ([0.5], False, ())
    assert lean.fields(2, 3, 5)["pathq"] is None and lean.fields(2, 3, 5)["pathv"] is None
    with pytest.raises(ValueError):
        _McQ(None, True, ())
    with pytest.raises(ValueError):
        _McQ(np.linspace(0, 1, 17), False, ())
    assert issubclass(McNavReport, McReport)


def q_case():
    """The inputs of the statistical anchor: plan 0 of the golden runs, the handover of the existing sampled checks (test_mc_cpu.w_case:
    cov_reference.handover_s0(x0, scale=0.1)), the reference's default gains, no clamp, no noise.  (p, par, x, u, s, L, S0, s(k) [K+1][5])"""
    p, par, x, u, s, d = _data()
    sl = slice(0, 1)
    L, _ = tr.gains(d, p.K)
    S0, _ = cr.handover_s0(x[0, 0], scale=0.1)
    cov = cr.propagate(d[sl], p.K, L[sl], S0[None])
    return p, par, x, u, s, L, S0, mgr.path_sigma(p, x[sl], u[sl], cov)[0]


def anchor(p, vals, gbar, sk):
    """(worst |Q_Phi(1) - gbar - s(k)| and worst |Q_0.5 - gbar| over the nodes 1..K, [5] each, in standard errors of the quantile
    estimator under the normal model, sqrt(p (1 - p) / S) / phi(z_p) s(k)); vals [S][K+1][5]"""
    S = vals.shape[0]
    p1 = NormalDist().cdf(1.0)
    rk = qr.ranks([p1, 0.5], S)
    q = qr.order_stats(vals, rk, axis=0)                                # [K+1][5][2]
    with np.errstate(all="ignore"):
        z1 = np.abs(q[1:, :, 0] - gbar[1:] - sk[1:]) / (qr.quantile_se(p1, S) * sk[1:])
        z0 = np.abs(q[1:, :, 1] - gbar[1:]) / (qr.quantile_se(0.5, S) * sk[1:])
    return z1.max(axis=0), z0.max(axis=0)


def test_per_node_quantiles_against_first_order_sigma_within_six_standard_errors():
    """8,192 flights of golden plan 0 through the C oracle's closed loop at the handover of the existing sampled checks, no clamp, no
    noise: at every node 1..K the Phi(1)-quantile of MASS and of THRUST minus the plan's own value against the first-order s(k) of
    tests/cov_reference.py, and the median minus the plan's value against 0, both within 6 standard errors of the quantile estimator
    under the normal model.  The reference flights stay within it at that handover as it is: it was not shrunk.  TILT and RATE are
    norms of near-zero vectors at many nodes, where first order says nothing: printed, not asserted (GLIDE likewise printed)."""
    from oracle import dynamics as od
    from successiveconvexification_amd.montecarlo import handover_factor, mc_draws
    p, par, x, u, s, L, S0, sk = q_case()
    N = Q_SAMPLES
    xi0, _ = mc_draws(N, p.K, Q_SEED)
    dx0 = xi0 @ handover_factor(S0).T
    _, _, xf, _, cmd = mr.chain(od, par, p, np.broadcast_to(x[0], (N,) + x[0].shape), np.broadcast_to(u[0], (N,) + u[0].shape),
                                np.full(N, float(s[0])), np.broadcast_to(L[0], (N,) + L[0].shape), dx0, 10)
    vals = qr.path_values(p, xf, cmd, u[0, 0])
    z1, z0 = anchor(p, vals, qr.plan_values(p, x[0], u[0]), sk)
    for f, name in enumerate(qr.COLUMNS):
        print("C oracle, plan 0, S = %d, seed %d, %s: worst |Q_Phi(1) - gbar - s(k)| %.2f SE, worst |Q_0.5 - gbar| %.2f SE over nodes 1..K%s"
              % (N, Q_SEED, name, z1[f], z0[f], "" if name in ("MASS", "THRUST") else "   (not asserted)"))
    for name in ("MASS", "THRUST"):
        assert z1[qr.IDX[name]] <= 6.0 and z0[qr.IDX[name]] <= 6.0, (name, z1, z0)
