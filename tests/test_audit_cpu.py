"""The segment audit and the back-offs taken from it, without a device: the CPU reference (tests/audit_reference.py) against the flight
check's reference and against the oracle's own runs in tests/golden/oracle_audit_runs.npz, the back-off rule's contract, and the three
bindings of the new symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import audit_reference as ar
import flight_reference as fr
import path_margin_reference as pr
from conftest import GOLDEN, ROOT

NEW = ("scvx_segment_audit_f64", "scvx_segment_audit_f64_host", "scvx_batch_segment_audit", "scvx_batch_audit_margins")
KINDS = ("thrust", "tilt")


def _problem():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_oracle_flight_runs", os.path.join(GOLDEN, "make_oracle_flight_runs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.flyable_problem()


@pytest.fixture(scope="module")
def runs():
    return np.load(os.path.join(GOLDEN, "oracle_audit_runs.npz")), np.load(os.path.join(GOLDEN, "oracle_flight_runs.npz")), _problem()


def test_the_fixture_audits_are_those_of_its_plans(runs):
    """every seg of the fixture re-derived from the plan stored beside it; the numbers the README quotes"""
    from oracle import dynamics as od
    a, g, p = runs
    nsub, tol = int(a["nsub"]), float(a["tol"])
    assert (nsub, float(a["gain"]), tol, float(a["cap"])) == (10, 1.5, 1e-7, 0.25) and a["dropped_runs"].tolist() == ["none"]
    par = od.Params(p)
    base, rep = ar.audit(od, p, g["x"], g["u"], g["sigma"], nsub, par)
    for t in range(2):
        assert np.array_equal(base[t], a["seg_%d" % t])
        for j in range(int(a["rounds_%d" % t])):
            k = "r%d_%d_" % (t, j)
            seg = ar.audit(od, p, a[k + "x"][None], a[k + "u"][None], a[k + "sigma"][None], nsub, par)[0][0]
            assert np.array_equal(seg, a[k + "seg"]), k
    v = [ar.violations(base[t], ("thrust", "glide", "tilt", "rate"), tol) for t in range(2)]
    print("base plans:", v)
    assert [v[t]["thrust"][0] for t in range(2)] == [4, 9] and [v[t]["tilt"][0] for t in range(2)] == [3, 3]
    assert abs(v[0]["thrust"][1] - 2.08e-4) < 5e-7 and abs(v[1]["thrust"][1] - 1.40e-4) < 5e-7
    assert abs(v[0]["tilt"][1] - 2.20e-4) < 5e-7 and abs(v[1]["tilt"][1] - 2.63e-4) < 5e-7
    assert max(v[t]["glide"][1] for t in range(2)) <= 2e-10 and all(v[t]["rate"][0] == 0 for t in range(2))
    # convex along a hold / monotone: never above their node values
    for t in range(2):
        un = np.linalg.norm(g["u"][t], axis=-1)
        assert base[t, :, ar.IDX["G_TMAX"]].max() <= (un - p.Tmax).max() + 1e-15
        # (a segment's last sample is its propagated end, which is the next node up to the segment's defect)
        assert base[t, :, ar.IDX["G_MASS"]].max() <= (p.mdry - g["x"][t, :, 0]).max() + base[t, :, ar.IDX["DEFECT"]].max()
    # the maxima over the segments are the PLAN-mode flight report, column for column, bit for bit
    assert np.array_equal(rep, g["report_plan"])
    for name, col in ar.report_from_seg(base).items():
        assert np.array_equal(col, rep[:, fr.IDX[name]]), name
    # at nsub 40 the figures move in the third digit
    b40 = ar.audit(od, p, g["x"], g["u"], g["sigma"], 40, par)[0]
    t40 = b40[..., ar.IDX["G_TILT"]].max(axis=1)
    print("tilt at nsub 40:", t40)
    assert abs(t40[0] - 2.2025e-4) < 5e-8 and abs(t40[1] - 2.70e-4) < 5e-7


def test_the_oracle_is_clean_within_three_rounds_and_one(runs):
    a, g, p = runs
    tol = float(a["tol"])
    need = [int(a["rounds_%d" % t]) for t in range(2)]
    assert need[0] <= 3 and need[1] <= 1, need
    for t in range(2):
        last = a["r%d_%d_seg" % (t, need[t] - 1)]
        assert all(n == 0 for n, _ in ar.violations(last, KINDS, tol).values()), ar.violations(last, KINDS, tol)
        for j in range(need[t] - 1):
            assert any(n for n, _ in ar.violations(a["r%d_%d_seg" % (t, j)], KINDS, tol).values())
        # the final mass does not drop
        assert a["r%d_%d_x" % (t, need[t] - 1)][-1, 0] >= g["x"][t, -1, 0]
    assert "".join("a" if v else "r" for v in a["r0_0_accepted"]) == "arrrrrrraaaaa" and len(a["r1_0_accepted"]) == 6
    assert a["r0_0_seg"][:, ar.IDX["G_TMIN"]].max() <= 0


def test_the_backoff_rule_and_its_contract(runs):
    """accumulation round over round as the fixture stores it, the contract of the entries, the thrust-band rule, caps, forced zeros,
    a NaN plan"""
    a, g, p = runs
    K = p.K
    gain, tol, cap = float(a["gain"]), float(a["tol"]), float(a["cap"])
    for t in range(2):
        lo, pm = np.zeros(K + 1), np.zeros((K + 1, 4))
        x, seg = g["x"][t], a["seg_%d" % t]
        for j in range(int(a["rounds_%d" % t])):
            k = "r%d_%d_" % (t, j)
            lo, pm = ar.backoff_rule(p, x, seg, lo, pm, KINDS, gain, tol, cap)
            assert np.array_equal(lo, a[k + "lo"]) and np.array_equal(pm, a[k + "pm"])
            pr.check_contract(p, pm)
            assert np.all(lo >= 0) and np.all(lo < p.Tmax - p.Tmin)              # the thrust-band rule with hi = 0
            assert not pm[:, [pr.MASS, pr.GLIDE, pr.RATE]].any()
            x, seg = a[k + "x"], a[k + "seg"]
        # back-offs only where a segment fails, at its two nodes
        e = ar.excess(a["seg_%d" % t][:, ar.IDX["G_TMIN"]], tol)
        assert np.array_equal(a["r%d_0_lo" % t], gain * e) and (e > 0).sum() >= (a["seg_%d" % t][:, ar.IDX["G_TMIN"]] > tol).sum() + 1
    # caps and forced zeros: every kind, a gain that drives everything into the cap
    x, seg = g["x"][0], np.abs(a["seg_0"]) + 1.0
    lo, pm = ar.backoff_rule(p, x, seg, np.zeros(K + 1), np.zeros((K + 1, 4)), ("thrust", "glide", "tilt", "rate"), 1e6, 0.0, 0.25)
    tggs, sqcm = pr.consts(p)
    pr.check_contract(p, pm)
    assert np.all(lo == 0.25 * (p.Tmax - p.Tmin))
    assert np.all(pm[:K, pr.TILT] == 0.25 * sqcm) and pm[K, pr.TILT] == 0 and np.all(pm[1:K, pr.RATE] == 0.25 * p.omMax)
    assert np.array_equal(pm[1:K, pr.GLIDE], 0.25 * (np.maximum(x[1:K, 1], 0.0) * (1.0 / tggs)))
    assert not pm[0, [pr.GLIDE, pr.RATE]].any() and not pm[K].any() and not pm[:, pr.MASS].any()
    # what is there already shows as negative G: nothing is added on top
    lo2, pm2 = ar.backoff_rule(p, x, -seg, lo, pm, ("thrust", "tilt"), 1.5, 1e-7, 0.25)
    assert np.array_equal(lo2, lo) and np.array_equal(pm2, pm)
    # a NaN in a selected column leaves the plan as it is; in another column it does not matter
    bad = a["seg_0"].copy()
    bad[7, ar.IDX["G_TILT"]] = np.nan
    l0, p0 = np.full(K + 1, 1e-5), np.zeros((K + 1, 4))
    l1, p1 = ar.backoff_rule(p, x, bad, l0, p0, KINDS, 1.5, 1e-7, 0.25)
    assert np.array_equal(l1, l0) and np.array_equal(p1, p0)
    l2, _ = ar.backoff_rule(p, x, bad, l0, p0, ("thrust",), 1.5, 1e-7, 0.25)
    assert (l2 > l0).any()
    with pytest.raises(AssertionError):
        ar.backoff_rule(p, x, bad, l0, p0, ("mass",), 1.5, 1e-7, 0.25)


def test_nan_sample_stays_in_its_segment():
    a = np.load(os.path.join(GOLDEN, "oracle_flight_runs.npz"))
    from oracle import dynamics as od
    p = _problem()
    x = a["x"].copy()
    x[1, 20, 9] = np.nan
    clean = ar.audit(od, p, a["x"], a["u"], a["sigma"], 2)[0]
    seg = ar.audit(od, p, x, a["u"], a["sigma"], 2)[0]
    state = [ar.IDX[n] for n in ("DEFECT", "G_MASS", "G_GLIDE", "G_TILT", "G_RATE", "QNORM")]
    assert np.isnan(seg[1, 20, state]).all() and np.isnan(seg[1, 19, ar.IDX["DEFECT"]])
    assert np.array_equal(seg[1, 19, 1:], clean[1, 19, 1:]) and np.array_equal(seg[1, 20, 5:8], clean[1, 20, 5:8])
    keep = np.ones((2, 50), bool)
    keep[1, 19:21] = False
    assert np.array_equal(seg[keep], clean[keep])


def test_header_binding_and_julia_carry_the_same_symbols():
    from py_call_recorder import header_params
    from successiveconvexification_amd import _calls, _lib, build
    import subprocess
    hdr = open(os.path.join(ROOT, "include", "scvx.h")).read()
    jl = open(os.path.join(ROOT, "julia", "ScvxAMD.jl")).read()
    par = header_params()
    for sym in NEW:
        assert sym in par and sym in _lib.SIGNATURES and ":" + sym in jl, sym
        assert len(par[sym]) == len(_lib.SIGNATURES[sym][1]), sym
    so = build.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    assert set(NEW) <= set(re.findall(r"\bT (scvx_[a-z0-9_]+)", out))
    # only functions were added: the ABI version stays; the Julia additions sit outside install!()
    assert int(re.search(r"#define SCVX_ABI_VERSION (\d+)", hdr).group(1)) == 4 == _lib.ABI_VERSION
    for fn in ("function segment_audit(cache::Cache", "function margins_from_audit!(b::Batch"):
        assert jl.index(fn) < jl.index("function install!")
    # the columns: header macros, binding and reference agree
    for i, n in enumerate(_lib.SEG_COLUMNS):
        assert int(re.search(r"#define SCVX_SEG_%s (\d+)" % n, hdr).group(1)) == i == ar.IDX[n]
    assert int(re.search(r"#define SCVX_SEG_N (\d+)", hdr).group(1)) == _lib.SEG_N == ar.SEG_N == len(_lib.SEG_COLUMNS)
    assert [n for n in _lib.FLIGHT_COLUMNS if n.startswith("G_")] == [n for n in _lib.SEG_COLUMNS if n.startswith("G_")]
    # the dispatcher's table is the header's parameter list and the binding's kinds
    for name, fields in _calls.AUDIT_TABLE.items():
        assert tuple(n for _, n in par[name][1:]) == fields, name
        assert len(_lib.SIGNATURES[name][1]) == len(fields) + 1
    assert _lib.SIGNATURES["scvx_batch_audit_margins"][1][2] is C.c_uint
    assert not set(_calls.AUDIT_TABLE) & set(_calls.TABLE)
    flat = re.sub(r"\s*\n \*\s*", " ", hdr)
    for word in ("substep boundaries only", "gain is a starting point", "ACCUMULATE", "mass is monotone", "have no back-off"):
        assert word in flat, word
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(sym in integ for sym in ("scvx_segment_audit_f64", "scvx_batch_audit_margins", "margins_from_audit!", "segment_audit_batch"))


def test_python_calls_lay_out_their_records_and_refuse_before_the_library():
    from py_call_recorder import Recorder, Unreachable, make_cache
    from successiveconvexification_amd import montecarlo as mc
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import SegmentReport, segment_audit_batch
    rec = Recorder()
    cache = make_cache(rec, 3, False)
    z = np.zeros
    rep = segment_audit_batch(cache, z((2, 4, 14)), z((2, 4, 3)), z(2))
    assert isinstance(rep, SegmentReport) and rep.seg.shape == (2, 3, 11) and rep.G_TMIN.shape == (2, 3) and len(rep.flight) == 2
    assert re.fullmatch(r"scvx_segment_audit_f64_host\(ctx=handle, B=2, K=3, x=<f8\[2, 4, 14\] crc=\w+, u=<f8\[2, 4, 3\] crc=\w+, "
                        r"sigma=<f8\[2\] crc=\w+, nsub=4, seg=<f8\[2, 3, 11\], report=<f8\[2, 16\]\)", rec.lines[-1]), rec.lines[-1]
    b = ScvxBatch.__new__(ScvxBatch)
    b.B, b.K, b._L, b.handle, b.cache = 2, 3, rec, C.c_void_p(2), cache
    assert b.audit(nsub=7).seg.shape == (2, 3, 11)
    assert rec.lines[-1] == "scvx_batch_segment_audit(b=handle, nsub=7, seg=<f8[2, 3, 11], report=<f8[2, 16])"
    assert b.margins_from_audit().shape == (2, 3, 11)
    assert rec.lines[-1] == "scvx_batch_audit_margins(b=handle, nsub=0, which=9, gain=1.5, tol=1e-07, cap=0.25, seg=<f8[2, 3, 11])"
    assert b.margins_from_audit(("thrust", "glide", "tilt", "rate"), gain=2, tol=0, cap=0.1, nsub=40, want_seg=False) is None
    assert rec.lines[-1] == "scvx_batch_audit_margins(b=handle, nsub=40, which=29, gain=2.0, tol=0.0, cap=0.1, seg=NULL)"
    n = len(rec.lines)
    b._L = Unreachable()
    for bad in (("mass",), ("thrust", "mass"), (), ("gimbal",), "thrust"):
        with pytest.raises(ValueError):
            b.margins_from_audit(bad)
        with pytest.raises(ValueError):
            b.harden(bad)
    with pytest.raises(ValueError):
        b.harden(restart="again")
    with pytest.raises(ValueError):
        b.harden(rounds=0)
    with pytest.raises(ValueError):
        segment_audit_batch(make_cache(Unreachable(), 3, False), z((2, 4, 13)), z((2, 4, 3)), z(2))
    assert len(rec.lines) == n
    # worst() and the summary
    seg = np.full((3, 4, 11), -1.0)
    seg[0, 2, ar.IDX["G_TILT"]] = 3e-4
    seg[1, 1, ar.IDX["G_TILT"]] = np.nan
    seg[2, :, ar.IDX["G_TMIN"]] = [1e-4, 2e-4, -1.0, 5e-8]
    r = SegmentReport(seg, np.zeros((3, 16)))
    val, k = r.worst("G_TILT")
    assert val[0] == 3e-4 and k[0] == 2 and np.isnan(val[1]) and k[1] == 1 and val[2] == -1.0
    s = mc.audit_summary(r, np.array([0, 3, 0]), 1e-7)
    assert s["n"] == 3 and s["converged"] == 2
    assert s["stats"]["G_TILT"] == {"plans": 0.5, "segments": 1 / 8, "max": 3e-4} and s["stats"]["G_TMIN"] == {"plans": 0.5, "segments": 2 / 8, "max": 2e-4}
    assert s["stats"]["G_MASS"] == {"plans": 0.0, "segments": 0.0, "max": -1.0}
    assert mc.audit_summary(seg, np.array([1, 1, 1]))["stats"]["G_TILT"] is None
    with pytest.raises(ValueError):
        mc.audit_summary(seg, np.zeros(2))
