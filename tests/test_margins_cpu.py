"""Thrust-band back-offs without a GPU: the three bindings (header, _lib.SIGNATURES, julia/ScvxAMD.jl) against each other, the
refusals of the host layer, the independent reference's own edits (tests/margin_reference.py) and the invariants of the committed
fixture tests/golden/oracle_margin_runs.npz (the CPU oracle's runs under back-offs)."""
import os
import re

import numpy as np
import pytest

import cov_reference as cr
import margin_reference as mr
from conftest import GOLDEN, ROOT

NEW = {"scvx_cov_path_sigma_f64": 11, "scvx_cov_path_sigma_f64_host": 11, "scvx_batch_set_thrust_margins": 3,
       "scvx_batch_get_thrust_margins": 3, "scvx_batch_thrust_margins_from_cov": 9, "scvx_batch_replan": 1}


def _flyable():
    from dataclasses import replace
    from oracle import model
    return replace(model.base_prob_scaled(), mdry=0.55, nuTol=1e-6, delTol=1e-3, imax=40, tf_guess=8.0)


def test_header_binding_and_julia_carry_the_same_symbols():
    from successiveconvexification_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "scvx.h")).read()
    jl = open(os.path.join(ROOT, "julia", "ScvxAMD.jl")).read()
    for sym, n in NEW.items():
        m = re.search(r"\bint %s\(([^;]*?)\);" % sym, hdr, flags=re.S)
        assert m, sym
        assert len(m.group(1).split(",")) == n, sym
        assert len(_lib.SIGNATURES[sym][1]) == n, sym
        j = re.search(r"ccall\(\(:%s, LIB\), Cint,\s*\(([^)]*)\)" % sym, jl, flags=re.S)
        assert j, sym
        assert len([a for a in j.group(1).split(",") if a.strip()]) == n, sym
    # the path-sigma call takes scvx_cov_propagate_f64's arguments up to report_dev, then psig
    cov = re.search(r"\bint scvx_cov_propagate_f64\(([^;]*?)\);", hdr, flags=re.S).group(1).split(",")
    ps = re.search(r"\bint scvx_cov_path_sigma_f64\(([^;]*?)\);", hdr, flags=re.S).group(1).split(",")
    assert [a.split()[-1] for a in ps[:-1]] == [a.split()[-1] for a in cov[:10]] and ps[-1].split()[-1] == "*psig_dev"
    mac = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define SCVX_PSIG_([A-Z_]+) (\d+)", hdr)}
    assert mac.pop("N") == 5 == _lib.PSIG_N == len(mr.PSIG_COLUMNS)
    assert mac == _lib.PSIG_INDEX and _lib.PSIG_COLUMNS == mr.PSIG_COLUMNS
    for name, i in _lib.PSIG_INDEX.items():
        assert int(re.search(r"const PSIG_%s = (\d+)" % name, jl).group(1)) == i
    # only functions were added: the ABI version and the struct mirrors stay
    assert int(re.search(r"#define SCVX_ABI_VERSION (\d+)", hdr).group(1)) == 4 == _lib.ABI_VERSION
    # outside install!(): that function's body is pinned to the reference's by test_abi_harness.py
    for fn in ("function robustify!(b::Batch", "function set_thrust_margins!(b::Batch", "replan!(b::Batch)"):
        assert jl.index(fn) < jl.index("function install!")
    assert "robustify" not in jl[jl.index("function install!"):]
    # the stated limits are in the header
    for word in ("FIRST ORDER", "only as good as Sigma_k", "2.5 - 3 sigma", "another local optimum", "ARE part of a checkpoint"):
        assert word in hdr, word


def test_the_core_keeps_consts_and_the_port_signature():
    """ipm::Consts is mirrored by oracle/port.py with ctypes and Solver::solve is called by oracle/scvx_port.cpp: neither may change"""
    core = open(os.path.join(ROOT, "successiveconvexification_amd", "csrc", "scvx_ipm_core.hpp")).read()
    m = re.search(r"struct Consts \{(.*?)\n\};", core, flags=re.S)
    assert m and "marg" not in m.group(1) and "lo" not in re.findall(r"\b[a-z]+\b", m.group(1))
    assert "SCVX_HD Result solve(cdptr xbar_, cdptr ubar_, cdptr endpoint_, dcptr D_,\n                         double rk_, cdptr ic, gptr work, bool warm = false) {" in core
    assert "SCVX_HD void set_margins(cgptr m)" in core
    # the two places that read the upper bound read the per-node array
    assert core.count("af * tmx[k]") == 2 and "af * C.Tmax" not in core


class _FakeLib:
    def __getattr__(self, name):
        raise AssertionError("the library must not be reached: %s" % name)


def test_host_layer_refusals_come_before_the_library():
    from successiveconvexification_amd import rocketland as rl
    from successiveconvexification_amd.batch import ScvxBatch
    b = ScvxBatch.__new__(ScvxBatch)
    b.B, b.K, b._L, b.handle = 3, 50, _FakeLib(), None
    with pytest.raises(ValueError):
        b.set_thrust_margins(np.zeros((3, 51)), None)
    with pytest.raises(ValueError):
        b.set_thrust_margins(None, 0.0)
    with pytest.raises(ValueError):
        b.set_thrust_margins(np.zeros((3, 50)), np.zeros((3, 50)))     # [B][K], not [B][K+1]
    with pytest.raises(ValueError):
        b.robustify(np.eye(14), rounds=0)
    with pytest.raises(ValueError):
        rl.robustify(None, None)


def test_reference_edits_are_the_two_row_blocks():
    from oracle import scvx, socp
    p = _flyable()
    K = p.K
    g = np.load(os.path.join(GOLDEN, "oracle_margin_runs.npz"))
    it = scvx.create_initial(p, 10, g["ic"][0, :3], g["ic"][0, 3:])
    base = socp.build(it.problem, it.x, it.u, it.endpoint, it.deriv, it.rk)
    z = np.zeros(K + 1)
    same = mr.build(it.problem, it.x, it.u, it.endpoint, it.deriv, it.rk, z, z)
    assert np.array_equal(same[4], base[4]) and (same[3] != base[3]).nnz == 0 and same[5:7] == base[5:7]
    lo, hi = g["lo"][0], g["hi"][0]
    ed = mr.build(it.problem, it.x, it.u, it.endpoint, it.deriv, it.rk, lo, hi)
    diff = np.flatnonzero(ed[4] != base[4])
    rows = np.concatenate([np.arange(K, 2 * K + 1)[hi > 0], np.arange(3 * K + 2, 4 * K + 3)[lo > 0]])
    assert np.array_equal(diff, rows)
    assert np.allclose(base[4][K:2 * K + 1] - ed[4][K:2 * K + 1], hi, rtol=0, atol=2.0 ** -52 * p.Tmax)   # one rounding of Tmax - hi
    assert np.allclose(base[4][3 * K + 2:4 * K + 3] - ed[4][3 * K + 2:4 * K + 3], lo, rtol=0, atol=2.0 ** -52 * p.Tmax)
    with pytest.raises(AssertionError):
        mr.build(it.problem, it.x, it.u, it.endpoint, it.deriv, it.rk, np.full(K + 1, 0.6 * (p.Tmax - p.Tmin)), np.full(K + 1, 0.6 * (p.Tmax - p.Tmin)))
    # the stored first subproblem satisfies the edited rows: the cone head and the linearised lower bound
    u = g["sub_u"][0]
    t = np.linalg.norm(u[:, :3], axis=1)
    un = np.linalg.norm(it.u[:, :3], axis=1)
    low = np.einsum("ki,ki->k", it.u[:, :3] / un[:, None], u[:, :3] - it.u[:, :3]) - ((p.Tmin + lo) - un)
    print("first subproblem: (Tmax - hi) - |u| >= %.2e, linearised lower row >= %.2e" % ((p.Tmax - hi - t).min(), low.min()))
    assert (t <= p.Tmax - hi + 1e-8).all() and (low >= -1e-8).all()


def test_fixture_invariants():
    p = _flyable()
    g = np.load(os.path.join(GOLDEN, "oracle_margin_runs.npz"))
    n = len(g["plans"])
    assert n >= 1 and g["plans"][0] == 0 and set(g["plans"]) | set(g["dropped"]) == {0, 1}
    lo, hi = g["lo"], g["hi"]
    assert np.array_equal(lo, hi) and np.array_equal(lo, np.minimum(float(g["nsigma"]) * g["psig"][:, :, 4], float(g["clip"])))
    assert (lo[:, 0] == 0).all() and (lo[:, 1:] > 0).all() and (lo + hi < p.Tmax - p.Tmin).all()
    e = np.abs(g["psig"] - g["psig_ld"]).max()
    print("psig float64 vs longdouble %.2e of %.2e" % (e, g["psig"].max()))
    assert e <= 1e-10 * g["psig"].max()
    # the base plans ride both bounds; under back-offs both runs keep the band at every node and regain the headroom
    base = g["base_rep"]
    assert (base[:, cr.IDX["N_TMIN"]] < 1e-4).all() and (base[:, cr.IDX["N_TMAX"]] < 1e-4).all()
    for name in ("guess", "replan"):
        bl, bh = zip(*(mr.band_margins(p, g[name + "_u"][i], lo[i], hi[i]) for i in range(n)))
        rep = g[name + "_rep"]
        acc = g[name + "_accepted"]
        print("%s: band held to %.1e / %.1e; N_TMIN %s N_TMAX %s; final mass %s; steps %s"
              % (name, -min(min(bl), 0), -min(min(bh), 0), rep[:, cr.IDX["N_TMIN"]], rep[:, cr.IDX["N_TMAX"]], g[name + "_x"][:, -1, 0],
                 (acc >= 0).sum(axis=1)))
        assert min(bl) >= -1e-6 and min(bh) >= -1e-6
        assert (rep[:, cr.IDX["N_TMIN"]] >= 2.0).all() and (rep[:, cr.IDX["N_TMAX"]] >= 2.0).all()
        assert (acc[:, 0] == 1).all()                                   # the first step is accepted through the rho = NaN branch
        last = (acc >= 0).sum(axis=1) - 1
        assert all(acc[i, last[i]] == 1 for i in range(n))             # a run ends on an accepted step
        cnu, cdel = g[name + "_cnu"], g[name + "_cdel"]
        assert all(cnu[i, last[i]] <= p.nuTol and cdel[i, last[i]] <= p.delTol for i in range(n))
        assert (g[name + "_x"][:, -1, 0] < g["base_x"][:, -1, 0]).all()   # headroom costs propellant
    assert ((g["replan_accepted"] >= 0).sum(axis=1) <= (g["guess_accepted"] >= 0).sum(axis=1)).all()
    # the per-node s of a margined plan, from the same reference
    assert g["guess_psig"].shape == (n, p.K + 1, 5) and np.isfinite(g["guess_psig"]).all()


def test_path_sigma_reference_against_the_report():
    """the per-node s reproduce the report's S_THRUST and margins exactly (same reference, same arithmetic), and a NaN poisons its row"""
    import track_reference as tr
    from oracle import dynamics as od
    p = _flyable()
    f = np.load(os.path.join(GOLDEN, "oracle_flight_runs.npz"))
    x, u, s = f["x"], f["u"], f["sigma"]
    _, d = od.linearize(od.Params(p), x, u, s, 1.0 / (p.K + 1), 10)
    L, _ = tr.gains(d, p.K)
    S0 = np.stack([cr.handover_s0(x[b, 0], 0, 1e-3)[0] for b in range(2)])
    rep, cov, _ = cr.run(p, x, u, d, p.K, L, S0)
    ps = mr.path_sigma(p, x, u, cov)
    assert np.array_equal(ps[:, :, 4].max(axis=1), rep[:, cr.IDX["S_THRUST"]]) and not ps[:, 0].any()
    t = np.linalg.norm(u[:, 1:, :3], axis=-1)
    with np.errstate(divide="ignore"):
        assert np.array_equal((-(p.Tmin - t) / ps[:, 1:, 4]).min(axis=1), rep[:, cr.IDX["N_TMIN"]])
        assert np.array_equal((-(p.mdry - x[:, 1:, 0]) / ps[:, 1:, 0]).min(axis=1), rep[:, cr.IDX["N_MASS"]])
    g = np.load(os.path.join(GOLDEN, "oracle_margin_runs.npz"))
    assert np.array_equal(ps[list(g["plans"])], g["psig"])
    cn = cov.copy()
    cn[1, 20, 3, 3] = np.nan
    pn = mr.path_sigma(p, x, u, cn)
    assert np.isnan(pn[1]).all() and np.array_equal(pn[0], ps[0])
