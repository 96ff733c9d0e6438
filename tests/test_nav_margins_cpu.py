"""Back-offs taken from the navigation analysis, without a GPU: the reference of the per-node standard deviations under navigation
errors (tests/nav_margin_reference.py: margin_reference.path_sigma on the truth block of nav_reference.propagate) against the
covariance reference it must contain (N0 = 0) and against its own longdouble form; the fixture tests/golden/oracle_nav_margin_runs.npz
against a recomputation and against what it is there to show (a plan backed off 3 sigma by the covariance analysis keeps less than 2
once the law flies on an estimate, a plan backed off by the navigation analysis keeps more than 2.5); the three bindings (header,
_lib.SIGNATURES, julia/ScvxAMD.jl) against each other; the host layer's refusals of a malformed nav=(N0, H, rm).

Data: the two plans the oracle converges on (tests/golden/oracle_flight_runs.npz), tiles from oracle.dynamics.linearize."""
import os
import re
import subprocess
import types

import numpy as np
import pytest

import cov_reference as cr
import margin_reference as mr
import nav_margin_reference as nm
import nav_reference as nr
import track_reference as tr
from conftest import GOLDEN, ROOT
from test_cov_cpu import _data
from test_nav_cpu import WEIGHTS

NEW = {"scvx_nav_path_sigma_f64": 16, "scvx_nav_path_sigma_f64_host": 16, "scvx_batch_margins_from_nav": 14}
OLD = {"scvx_nav_cov_f64": 19, "scvx_nav_cov_f64_host": 19, "scvx_batch_nav_cov": 16, "scvx_cov_propagate_f64": 13,
       "scvx_cov_propagate_f64_host": 13, "scvx_cov_path_sigma_f64": 11, "scvx_cov_path_sigma_f64_host": 11,
       "scvx_batch_margins_from_cov": 10, "scvx_batch_thrust_margins_from_cov": 9}


def _fixture():
    return np.load(os.path.join(GOLDEN, "oracle_nav_margin_runs.npz"))


def _s0(x):
    return np.stack([cr.handover_s0(x[b, 0], 0, 1e-3)[0] for b in range(x.shape[0])])


@pytest.mark.parametrize("w", WEIGHTS)
def test_zero_navigation_error_gives_the_covariance_path_sigma(w):
    """N0 = 0: the estimate never errs, with a measurement or without, and psig is the covariance analysis' to the bound
    test_nav_cpu.py allows the z block it is read off (relative to the largest entry of the column's kind, as there)"""
    p, par, x, u, s, d = _data()
    S0 = _s0(x)
    H, rm = nm.position_model(x[0, 0])
    L, _ = tr.gains(d, p.K, *w)
    cov = cr.propagate(d, p.K, L, S0)
    ref = mr.path_sigma(p, x, u, cov)
    rld = mr.path_sigma(p, x, u, cr.propagate(d, p.K, L, S0, dtype=np.longdouble), np.longdouble)
    e_ref = float(np.abs(ref - rld).max() / np.abs(rld).max())
    bound = 1e-13 if w == WEIGHTS[0] else max(1e-13, 4.0 * e_ref)
    for Hm, r in ((None, None), (H, rm)):
        ps = nm.path_sigma(p, x, u, d, p.K, L, S0, np.zeros((14, 14)), Hm, r)
        e = float(np.abs(ps - ref).max() / np.abs(ref).max())
        print("weights %s, m = %d: navigation psig vs covariance psig %.2e (float64 vs longdouble %.2e, bound %.2e)"
              % (w, 0 if Hm is None else 3, e, e_ref, bound))
        assert e <= bound
        assert ps.shape == (2, p.K + 1, 5) and not ps[:, 0].any() and np.isfinite(ps).all() and (ps[:, 1:, 4] > 0).all()


@pytest.mark.parametrize("w", WEIGHTS)
def test_float64_against_longdouble_and_what_the_report_is_made_of(w):
    p, par, x, u, s, d = _data()
    S0 = _s0(x)
    H, rm = nm.position_model(x[0, 0])
    L, _ = tr.gains(d, p.K, *w)
    noise = np.random.default_rng(5).uniform(0.0, 1e-8, 14)
    for Hm, r, nz in ((None, None, None), (H, rm, None), (H, rm, noise)):
        ps = nm.path_sigma(p, x, u, d, p.K, L, S0, S0, Hm, r, nz)
        pld = nm.path_sigma(p, x, u, d, p.K, L, S0, S0, Hm, r, nz, dtype=np.longdouble)
        j64, _, cond = nr.propagate(d, p.K, L, S0, S0, Hm, r, nz)
        jld, _, _ = nr.propagate(d, p.K, L, S0, S0, Hm, r, nz, np.longdouble)
        E = np.abs(j64[:, :, :17, :17] - jld[:, :, :17, :17]).reshape(2, -1).max(axis=1).astype(np.float64)
        e = float(np.abs(ps - pld).max() / np.abs(pld).max())
        print("weights %s m = %d w %s: psig float64 vs longdouble %.2e of the largest, truth block %.2e of the joint's largest, cond(S) %.2e"
              % (w, 0 if Hm is None else 3, nz is not None, e, E.max() / float(np.abs(jld).max()), cond.max()))
        if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps:
            # the variances c' Xi[z z] c move by no more than |c|_1^2 times what the truth block itself moves (the reference's own
            # float64 error), plus the roundings of the quadratic form (3 terms) and of one square root taken twice
            dv = np.abs(ps.astype(np.longdouble) ** 2 - pld ** 2).astype(np.float64)
            yard = nm.variance_yardstick(p, x, u, E) + 16 * 2.0 ** -52 * (pld ** 2).astype(np.float64)
            print("   variances: worst difference over its yardstick %.2f" % (dv / np.where(yard > 0, yard, 1.0)).max())
            assert (dv <= yard).all()
        assert not ps[:, 0].any() and np.isfinite(ps).all()
        # the same numbers as the report's: S_THRUST is the largest s_T, N_TMIN the smallest headroom over s_T
        rep = nr.run(p, x, u, d, p.K, L, S0, S0, Hm, r, nz)["report"]
        assert np.array_equal(ps[:, :, nm.THRUST].max(axis=1), rep[:, cr.IDX["S_THRUST"]])
        t = np.linalg.norm(u[:, 1:, :3], axis=-1)
        assert np.array_equal((-(p.Tmin - t) / ps[:, 1:, nm.THRUST]).min(axis=1), rep[:, cr.IDX["N_TMIN"]])
    # navigation errors widen every column; a NaN in one trajectory's N0 poisons its rows, and only them
    ps = nm.path_sigma(p, x, u, d, p.K, L, S0, S0, H, rm)
    pc = mr.path_sigma(p, x, u, cr.propagate(d, p.K, L, S0))
    assert (ps[:, 1:, 1:] >= pc[:, 1:, 1:] * (1 - 1e-9)).all() and (ps[:, 2:, nm.THRUST] > pc[:, 2:, nm.THRUST]).all()
    N0 = S0.copy()
    N0[1, 3, 3] = np.nan
    bad = nm.path_sigma(p, x, u, d, p.K, L, S0, N0, H, rm)
    assert np.isnan(bad[1]).all() and np.array_equal(bad[0], ps[0])


def test_fixture_is_reproduced_and_says_what_it_is_there_to_say():
    p, par, x, u, s, d = _data()
    g = _fixture()
    K = p.K
    assert np.array_equal(g["base_x"], x) and np.array_equal(g["base_u"], u)
    S0 = _s0(x)
    H, rm = nm.position_model(x[0, 0])
    assert np.array_equal(g["S0"], S0) and np.array_equal(g["N0"], S0) and np.array_equal(g["H"], H) and np.array_equal(g["rm"], rm)
    assert H.shape == (3, 14) and np.array_equal(H[:, 1:4], np.eye(3)) and np.count_nonzero(H) == 3
    L, _ = tr.gains(d, K)
    ps = nm.path_sigma(p, x, u, d, K, L, S0, S0, H, rm)
    assert np.array_equal(ps, g["psig_nav"])
    assert np.array_equal(nm.path_sigma(p, x, u, d, K, L, S0, S0, H, rm, dtype=np.longdouble).astype(np.float64), g["psig_nav_ld"])
    assert np.array_equal(mr.path_sigma(p, x, u, cr.propagate(d, K, L, S0)), g["psig_cov"])
    assert not g["psig_nav"][:, 0].any()
    ratio = g["psig_nav"][:, 1:] / g["psig_cov"][:, 1:]
    print("navigation / covariance s, mean over nodes: thrust %s, tilt %s; largest thrust ratio %s"
          % (ratio[:, :, 4].mean(axis=1), ratio[:, :, 2].mean(axis=1), ratio[:, :, 4].max(axis=1)))
    assert (ratio[:, :, 4].mean(axis=1) > 1.5).all() and (ratio[:, :, 2].mean(axis=1) > 2.0).all()
    # plan 0 is replanned under both sets of back-offs; a plan the oracle does not converge on is named
    n = len(g["plans"])
    assert n >= 1 and g["plans"][0] == 0 and set(g["plans"]) | set(g["dropped"]) == {0, 1}
    kept = list(g["plans"])
    cap = float(g["cap"]) * (p.Tmax - p.Tmin)
    assert np.array_equal(g["nav_lo"], np.minimum(float(g["nsigma"]) * g["psig_nav"][kept, :, 4], cap))
    assert np.array_equal(g["cov_lo"], np.minimum(float(g["nsigma"]) * g["psig_cov"][kept, :, 4], cap))
    tmin, tmax = cr.IDX["N_TMIN"], cr.IDX["N_TMAX"]
    for name in ("nav", "cov"):
        acc = g[name + "_accepted"]
        steps = (acc >= 0).sum(axis=1)
        rep = g[name + "_navrep_cov"]
        print("%s back-offs: steps %s (accepted %s), final mass %s; navigation report N_TMIN %s N_TMAX %s, covariance report %s / %s; "
              "expected outside of the band per 256 flights %s (base %s)"
              % (name, steps, (acc == 1).sum(axis=1), g[name + "_x"][:, -1, 0], rep[:, tmin], rep[:, tmax], g[name + "_covrep"][:, tmin],
                 g[name + "_covrep"][:, tmax], g[name + "_outside"], g["base_outside"][kept]))
        assert steps[0] == 3 and (acc[0, :3] == 1).all()
        last = steps - 1
        assert all(g[name + "_cnu"][i, last[i]] <= p.nuTol and g[name + "_cdel"][i, last[i]] <= p.delTol for i in range(n))
        bl, bh = mr.band_margins(p, g[name + "_u"][0], g[name + "_lo"][0], g[name + "_lo"][0])
        assert bl >= -1e-6 and bh >= -1e-6
        assert (g[name + "_x"][:, -1, 0] < x[kept, -1, 0]).all()          # headroom costs propellant
        # the stored figures of the replanned plan are the reference's own
        assert abs(nm.outside_band(p, g[name + "_u"][0], g[name + "_psig_nav"][0]) - g[name + "_outside"][0]) <= 1e-9 * g[name + "_outside"][0]
    nav, cov = g["nav_navrep_cov"][0], g["cov_navrep_cov"][0]
    assert nav[tmin] >= 2.5 and nav[tmax] >= 2.5
    assert min(cov[tmin], cov[tmax]) < 2.0
    # ... while the covariance report of that plan still shows the headroom it was given
    assert g["cov_covrep"][0, tmin] >= 2.5 and g["cov_covrep"][0, tmax] >= 2.5
    assert g["nav_outside"][0] < g["cov_outside"][0] < g["base_outside"][0]
    assert g["nav_x"][0, -1, 0] < g["cov_x"][0, -1, 0]                     # the wider back-offs cost more


def test_header_binding_and_julia_carry_the_same_symbols():
    from successiveconvexification_amd import _lib, build
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
    # the path-sigma call takes scvx_nav_cov_f64's arguments up to navrep_dev, then psig; the batch call those of margins_from_cov with
    # the navigation model behind S0
    navc = re.search(r"\bint scvx_nav_cov_f64\(([^;]*?)\);", hdr, flags=re.S).group(1).split(",")
    ps = re.search(r"\bint scvx_nav_path_sigma_f64\(([^;]*?)\);", hdr, flags=re.S).group(1).split(",")
    assert [a.split()[-1] for a in ps[:-1]] == [a.split()[-1] for a in navc[:15]] and ps[-1].split()[-1] == "*psig_dev"
    mc = [a.split()[-1] for a in re.search(r"\bint scvx_batch_margins_from_cov\(([^;]*?)\);", hdr, flags=re.S).group(1).split(",")]
    mn = [a.split()[-1] for a in re.search(r"\bint scvx_batch_margins_from_nav\(([^;]*?)\);", hdr, flags=re.S).group(1).split(",")]
    assert mn == mc[:5] + ["*N0", "m", "*H", "*rm"] + mc[5:]
    import ctypes as C
    assert _lib.SIGNATURES["scvx_batch_margins_from_nav"][1][12] is C.c_uint and _lib.SIGNATURES["scvx_batch_margins_from_nav"][1][6] is C.c_int
    so = build.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    exported = set(re.findall(r"\bT (scvx_[a-z0-9_]+)", out))
    assert set(NEW) <= exported, set(NEW) - exported
    # only functions were added: the ABI version stays; the Julia additions sit outside install!()
    assert int(re.search(r"#define SCVX_ABI_VERSION (\d+)", hdr).group(1)) == 4 == _lib.ABI_VERSION
    for fn in ("function margins_from_nav!(b::Batch", "margins_from_nav(b::Batch", "function nav_path_sigma(cache::Cache"):
        assert jl.index(fn) < jl.index("function install!")
    assert "margins_from_nav" not in jl[jl.index("function install!"):]
    # the header says what exists now and states the limits
    for word in ("scvx_batch_margins_from_nav below", "FIRST ORDER", "optimal gain for the stated model", "no sigma at node 0",
                 "measurement at node K", "tan(gammaGs) times as many sigma", "2.7 - 3 sigma", "not its estimate"):
        assert word in re.sub(r"\s*\n \*\s*", " ", hdr), word
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(sym in integ for sym in ("scvx_nav_path_sigma_f64", "scvx_batch_margins_from_nav", "margins_from_nav!", "nav_path_sigma_batch"))


class _FakeLib:
    def __getattr__(self, name):
        raise AssertionError("the library must not be reached: %s" % name)


def test_a_malformed_navigation_model_is_refused_before_the_library():
    from successiveconvexification_amd import rocketland as rl
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import _nav_arg, nav_path_sigma_batch
    from successiveconvexification_amd.montecarlo import measurement_rows
    b = ScvxBatch.__new__(ScvxBatch)
    b.B, b.K, b._L, b.handle = 3, 50, _FakeLib(), None
    S0 = np.eye(14)
    H = measurement_rows("r")
    rm = np.full(3, 1e-8)
    bad = [(S0, H), (S0, H, rm, None), S0, (S0, H, 0.0), (S0, H, np.array([1e-8, -1e-8, 1e-8])), (S0, H, np.array([1e-8, np.nan, 1e-8])),
           (S0, H, np.full(2, 1e-8)), (S0, H[:, :13], rm), (S0, H.T, rm), (S0, np.ones(14), 1e-8), (S0, np.eye(14)[[0] * 15], 1e-8),
           (None, H, rm), (np.eye(13), H, rm), (S0, np.where(H > 0, np.inf, 0.0), rm), (S0, H, None)]
    for nav in bad:
        with pytest.raises(ValueError):
            _nav_arg(nav, 3)
        with pytest.raises(ValueError):
            b.robustify(S0, nav=nav)
        with pytest.raises(ValueError):
            b.path_sigma(S0, nav=nav)
        if isinstance(nav, tuple) and len(nav) == 3:
            with pytest.raises(ValueError):
                b.margins_from_nav(S0, *nav)
    with pytest.raises(ValueError):
        b.robustify(S0, nav=(S0, H, rm), constraints=("gimbal",))
    with pytest.raises(ValueError):
        b.robustify(S0, nav=(S0, H, rm), rounds=0)
    with pytest.raises(ValueError):
        b.margins_from_nav(S0, S0, H, rm, constraints=())
    with pytest.raises(ValueError):
        rl.robustify(None, None, nav=(S0, H, rm))                      # S0 is required
    # a good one comes back as the library wants it: N0 broadcast to the batch, a scalar rm to m values; H None is m = 0
    n0, m, Hm, rv = _nav_arg((np.full(14, 2.0), H, 1e-8), 3)
    assert n0.shape == (3, 14, 14) and np.array_equal(n0[1], 4.0 * np.eye(14)) and m == 3 and np.array_equal(Hm, H) and np.array_equal(rv, rm)
    assert Hm.flags.c_contiguous and rv.flags.c_contiguous and n0.flags.c_contiguous
    assert _nav_arg((S0, None, None), 2)[1:] == (0, None, None)
    # the one-shot call checks its model before the library too
    cache = types.SimpleNamespace(nu=3, _L=_FakeLib(), handle=None)
    z = np.zeros
    for Hb, rb in ((H[:, :13], rm), (H, np.full(2, 1e-8)), (H, None)):
        with pytest.raises(ValueError):
            nav_path_sigma_batch(cache, z((2, 51, 14)), z((2, 51, 3)), z((2, 50, 21, 14)), z((2, 50, 3, 17)), S0, S0, Hb, rb)
    with pytest.raises(ValueError):
        nav_path_sigma_batch(cache, z((2, 51, 14)), z((2, 51, 3)), z((2, 50, 21, 14)), z((2, 50, 3, 16)), S0, S0, H, rm)
