"""Path-constraint back-offs without a GPU: the three bindings (header, _lib.SIGNATURES, julia/ScvxAMD.jl) against each other, the
refusals of the host layer, the independent reference's own edits (tests/path_margin_reference.py), the invariants of the committed
fixtures tests/golden/oracle_path_margin_runs.npz and oracle_path_margin_k100.npz (the CPU oracle under back-offs) and the CPU twin
of the conic solve (tests/path_margin_port.cpp: the kernel's interior-point core with a one-lane host executor and
Solver::set_path_margins) against the independent oracle.

Bounds of the twin-against-oracle comparison: those of test_gpu_margins.test_one_subproblem_with_backoffs_against_the_independent_
oracle (both sides at 1e-9: 2e-5 on the minimiser, 1e-8 relative on the objective).  Every comparison prints its figures first."""
import ctypes as C
import os
import re
import subprocess
from dataclasses import replace

import numpy as np
import pytest

import path_margin_reference as pr
from conftest import GOLDEN, ROOT

NEW = {"scvx_batch_set_path_margins": 2, "scvx_batch_get_path_margins": 2, "scvx_batch_margins_from_cov": 10}
_dp = C.POINTER(C.c_double)
D100 = 1.0434e-5      # twin-to-oracle distance on group "k100": see test_twin_with_backoffs_against_the_independent_oracle


def _flyable(K=50, fins=False):
    from oracle import model
    if fins:
        return replace(model.base_prob_fin_scaled(), mdry=0.55, tf_guess=8.0)
    return replace(model.base_prob_scaled(), mdry=0.55, nuTol=1e-6, delTol=1e-3, imax=40, tf_guess=8.0, K=K)


def _fixture(name=None):
    """the fixture that holds group `name`: "k100" has a file of its own (make_oracle_path_margin_runs.py --k100)"""
    return np.load(os.path.join(GOLDEN, "oracle_path_margin_k100.npz" if name == "k100" else "oracle_path_margin_runs.npz"))


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
    assert "unsigned which" in re.search(r"\bint scvx_batch_margins_from_cov\(([^;]*?)\);", hdr, flags=re.S).group(1)
    assert _lib.SIGNATURES["scvx_batch_margins_from_cov"][1][8] is C.c_uint
    mac = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define SCVX_PMARG_([A-Z_]+) (\d+)", hdr)}
    assert mac.pop("N") == 4 == _lib.PMARG_N == len(pr.KINDS)
    assert mac == _lib.PMARG_INDEX and tuple(n.lower() for n in _lib.PMARG_COLUMNS) == pr.KINDS
    assert (pr.MASS, pr.GLIDE, pr.TILT, pr.RATE) == tuple(_lib.PMARG_INDEX[n] for n in ("MASS", "GLIDE", "TILT", "RATE"))
    # the path columns of psig are the path back-offs' columns
    assert all(_lib.PSIG_INDEX[n] == i for n, i in _lib.PMARG_INDEX.items())
    bits = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define SCVX_MARGIN_([A-Z]+) (\d+)u", hdr)}
    assert bits.pop("all") == 31 == sum(bits.values()) and bits == _lib.MARGIN_BITS
    for name, i in list(_lib.PMARG_INDEX.items()):
        assert int(re.search(r"const PMARG_%s = (\d+)" % name, jl).group(1)) == i
    for name, v in _lib.MARGIN_BITS.items():
        assert int(re.search(r"const MARGIN_%s = UInt32\((\d+)\)" % name.upper(), jl).group(1)) == v
    # only functions were added: the ABI version stays; the Julia additions sit outside install!()
    assert int(re.search(r"#define SCVX_ABI_VERSION (\d+)", hdr).group(1)) == 4 == _lib.ABI_VERSION
    for fn in ("function set_path_margins!(b::Batch", "function path_margins(b::Batch", "function margins_from_cov!(b::Batch"):
        assert jl.index(fn) < jl.index("function install!")
    # what is out of scope is said in the header
    for word in ("OUT OF SCOPE", "gimbal", "dynamic-pressure", "fin cone", "navigation analysis"):
        assert word in hdr, word


def test_the_core_keeps_its_interfaces_and_reads_the_arrays_at_two_sites_each():
    """what the CPU port depends on (ipm::Consts, solve()'s argument list, set_margins) stays, and the three constant terms are no
    longer formed from C; the patterns allow for any layout of the source text"""
    core = open(os.path.join(ROOT, "successiveconvexification_amd", "csrc", "scvx_ipm_core.hpp")).read()
    flat = re.sub(r"\s+", " ", core)
    m = re.search(r"struct Consts \{(.*?)\n\};", core, flags=re.S)
    assert m and "pmarg" not in m.group(1) and "pth" not in m.group(1)
    assert re.search(r"Result solve\(cdptr \w+, cdptr \w+, cdptr \w+, dcptr \w+, double \w+, cdptr \w+, gptr \w+, bool \w+ = false\)", flat)
    assert re.search(r"void set_margins\(cgptr \w+\)", flat) and re.search(r"void set_path_margins\(cgptr \w+\)", flat)
    # the constants are read through the per-node values: two sites each (cone_map and small_gather), and nowhere from C
    for old in (r"af \* C\.sqcm", r"af \* C\.omMax", r"af \* C\.mdry"):
        assert not re.search(old, flat), old
    for new in (r"af \* pth\[4 \* \w \+ 2\]", r"af \* pth\[4 \* \w \+ 3\]", r"af \* pth\[4 \* \w\]", r"\* C\.itan - af \* pth\[4 \* \w \+ 1\]"):
        assert len(re.findall(new, flat)) == 2, new
    assert len(re.findall(r"\bgptr pth;", flat)) == 1            # one pointer to the four per-node values


class _FakeLib:
    def __getattr__(self, name):
        raise AssertionError("the library must not be reached: %s" % name)


def test_host_layer_refusals_come_before_the_library():
    from successiveconvexification_amd import rocketland as rl
    from successiveconvexification_amd.batch import ScvxBatch
    b = ScvxBatch.__new__(ScvxBatch)
    b.B, b.K, b._L, b.handle = 3, 50, _FakeLib(), None
    with pytest.raises(ValueError):
        b.set_path_margins(tilt=np.zeros((3, 50)))          # [B][K], not [B][K+1]
    with pytest.raises(ValueError):
        b.set_path_margins(mass=np.zeros((2, 51)))
    for bad in ((), ("gimbal",), "tilt", ("thrust", "fin"), "everything"):
        with pytest.raises(ValueError):
            b.robustify(np.eye(14), constraints=bad)
    with pytest.raises(ValueError):
        b.robustify(np.eye(14), rounds=0, constraints="all")
    with pytest.raises(ValueError):
        b.margins_from_cov(np.eye(14), constraints=("drag",))
    with pytest.raises(ValueError):
        rl.robustify(None, None, constraints="all")
    assert ScvxBatch._margin_mask("all") == 31 and ScvxBatch._margin_mask(("thrust",)) == 1 and ScvxBatch._margin_mask(["tilt", "thrust"]) == 9


def test_broadcast_values_get_the_forced_zeros():
    from successiveconvexification_amd.batch import ScvxBatch
    got = {}

    class Lib:
        def scvx_batch_set_path_margins(self, h, p):
            got["pm"] = None if p is None else np.ctypeslib.as_array(p, (2 * 10 * 4,)).reshape(2, 10, 4).copy()
            return 0

    b = ScvxBatch.__new__(ScvxBatch)
    b.B, b.K, b._L, b.handle = 2, 9, Lib(), None
    b._chk = lambda rc, what: None
    b.set_path_margins(mass=0.1, glide=0.2, tilt=np.full(10, 0.3), rate=0.4)
    pm = got["pm"]
    pr.check_contract(_flyable(9), pm[0])
    assert pm[0, 0].tolist() == [0.0, 0.0, 0.3, 0.0] and pm[1, 9].tolist() == [0.1, 0.0, 0.0, 0.0] and pm[1, 4].tolist() == [0.1, 0.2, 0.3, 0.4]
    full = np.full((2, 10), 0.3)
    b.set_path_margins(tilt=full)                           # a full array is passed as it is: the library judges it
    assert np.array_equal(got["pm"][:, :, 2], full) and not got["pm"][:, :, [0, 1, 3]].any()
    b.set_path_margins()
    assert got["pm"] is None


def test_reference_edits_are_the_four_row_blocks():
    from oracle import scvx, socp
    g = _fixture()
    p = _flyable()
    K = p.K
    tggs, sqcm = pr.consts(p)
    it = scvx.create_initial(p, 10, g["k50_ic"][0, :3], g["k50_ic"][0, 3:])
    base = socp.build(it.problem, it.x, it.u, it.endpoint, it.deriv, it.rk)
    same = pr.build(it.problem, it.x, it.u, it.endpoint, it.deriv, it.rk, np.zeros((K + 1, 4)))
    assert np.array_equal(same[2], base[2]) and np.array_equal(same[4], base[4]) and (same[1] != base[1]).nnz == 0 and (same[3] != base[3]).nnz == 0
    assert same[5:7] == base[5:7]
    pm = g["k50_pm"][0]
    ed = pr.build(it.problem, it.x, it.u, it.endpoint, it.deriv, it.rk, pm)
    n0 = 14 * (K + 1) + 3 * (K + 1) + 25 + 14 * K
    rows_b = np.concatenate([n0 + np.flatnonzero(pm[:K, pr.GLIDE]), n0 + K + np.flatnonzero(pm[:K, pr.TILT]), n0 + 2 * K + np.flatnonzero(pm[:K, pr.RATE])])
    assert np.array_equal(np.flatnonzero(ed[2] != base[2]), rows_b) and len(rows_b) == 3
    assert np.array_equal(np.flatnonzero(ed[4] != base[4]), np.flatnonzero(pm[1:, pr.MASS])) and np.count_nonzero(pm[:, pr.MASS]) == 1
    assert (ed[1] != base[1]).nnz == 0 and (ed[3] != base[3]).nnz == 0 and np.array_equal(ed[0], base[0])
    assert np.array_equal(ed[2][n0:n0 + K], -pm[:K, pr.GLIDE]) and np.array_equal(ed[2][n0 + K:n0 + 2 * K], sqcm - pm[:K, pr.TILT])
    assert np.array_equal(ed[2][n0 + 2 * K:n0 + 3 * K], p.omMax - pm[:K, pr.RATE]) and np.array_equal(ed[4][:K], -(p.mdry + pm[1:, pr.MASS]))
    # with the thrust edits of margin_reference on top
    lo = np.full(K + 1, 1e-3)
    both = pr.build(it.problem, it.x, it.u, it.endpoint, it.deriv, it.rk, pm, lo, 2 * lo)
    assert np.array_equal(both[2], ed[2]) and np.array_equal(both[4][K:2 * K + 1], p.Tmax - 2 * lo) and np.array_equal(both[4][:K], ed[4][:K])
    # the contract's refusals
    for k, c, v in ((K, pr.TILT, 0.1), (K, pr.GLIDE, 0.1), (K, pr.RATE, 0.1), (0, pr.MASS, 0.1), (0, pr.GLIDE, 0.1), (0, pr.RATE, 0.1),
                    (3, pr.TILT, sqcm), (3, pr.RATE, p.omMax), (3, pr.MASS, p.mwet - p.mdry), (3, pr.TILT, -1e-9), (3, pr.GLIDE, np.nan), (3, pr.MASS, np.inf)):
        bad = np.zeros((K + 1, 4))
        bad[k, c] = v
        with pytest.raises(AssertionError):
            pr.check_contract(p, bad)
    ok = np.zeros((K + 1, 4))
    ok[0, pr.TILT] = 0.1                                    # q_0 is free
    pr.check_contract(p, ok)


def test_fixture_invariants():
    import cov_reference as cr
    for name, p in (("k9", _flyable(9)), ("k50", _flyable()), ("k50f", _flyable()), ("fin", _flyable(fins=True)), ("k100", _flyable(100))):
        g = _fixture(name)
        pm, x = g[name + "_pm"], g[name + "_x"]
        assert pm.shape == (3, p.K + 1, 4) and (g[name + "_kinds"] == 15).all()
        assert len({pm[t].tobytes() for t in range(3)}) == 3                     # different back-offs per trajectory
        for t in range(3):
            pr.check_contract(p, pm[t])
            s = pr.slacks(p, x[t], pm[t])
            free = pr.slacks(p, x[t])
            print("%s start %d: smallest tightened slack per kind %s (of the true rows %s), violation %.1e"
                  % (name, t, s.min(axis=0), free.min(axis=0), -min(s.min(), 0.0)))
            act = (s < 1e-7) & (pm[t] > 0)
            assert (act.sum(axis=0) >= 1).all() and s.min() > -1e-8             # every kind active at a node or more, none violated
            assert (free[act] > 1e-4).all()                                      # ... and active because of its back-off: the true row is slack there
    assert sorted(_fixture("k100").files) == sorted("k100_" + k for k in ("ic", "pm", "kinds", "x", "u", "dsig", "nu", "pobj"))
    assert np.array_equal(_fixture("k100")["k100_ic"], _fixture()["k50_ic"])        # the three starts of "k50"
    # the complete run under the tilt back-offs of the base plan
    g = _fixture()
    p = _flyable()
    tggs, sqcm = pr.consts(p)
    assert "run0_x" in g.files
    pm = g["run0_pm"]
    assert np.array_equal(pm, pr.margins_from_sigma(p, np.load(os.path.join(GOLDEN, "oracle_flight_runs.npz"))["x"][0], g["base_psig_0"],
                                                    float(g["nsigma"]), float(g["cap"]), ("tilt",)))
    assert not pm[:, [pr.MASS, pr.GLIDE, pr.RATE]].any() and (pm[1:p.K, pr.TILT] > 0).all() and pm[p.K, pr.TILT] == 0
    seq = "".join("a" if a else "r" for a in g["run0_accepted"])
    viol = float(abs(pr.slacks(p, g["run0_x"], pm)[:, pr.TILT].min()))   # how exactly the oracle resolves the active cone: see the generator
    print("plan 0 under tilt back-offs: %d steps %s, final mass %.6f, N_TILT %.3g -> %.3f, tightened cone resolved to %.1e; dropped runs: %s"
          % (len(seq), seq, g["run0_x"][-1, 0], g["base_rep_0"][cr.IDX["N_TILT"]], g["run0_rep"][cr.IDX["N_TILT"]], viol, list(g["dropped_runs"])))
    assert seq == "arrrrrrraaaaa"
    assert g["run0_cnu"][-1] <= p.nuTol and g["run0_cdel"][-1] <= p.delTol
    assert viol == float(g["run0_viol"]) and 0 < viol < 1e-6
    assert g["base_rep_0"][cr.IDX["N_TILT"]] < 1e-4 and g["base_rep_1"][cr.IDX["N_TILT"]] < 1e-4
    assert g["run0_rep"][cr.IDX["N_TILT"]] >= 2.0
    assert abs(g["run0_x"][-1, 0] - 0.903985) < 1e-6
    # plan 1, on which the oracle converges as well (6 accepted steps): the same invariants
    pm1 = g["run1_pm"]
    flight = np.load(os.path.join(GOLDEN, "oracle_flight_runs.npz"))
    assert np.array_equal(pm1, pr.margins_from_sigma(p, flight["x"][1], g["base_psig_1"], float(g["nsigma"]), float(g["cap"]), ("tilt",)))
    s1 = pr.slacks(p, g["run1_x"], pm1)[:, pr.TILT]
    print("plan 1 under tilt back-offs: %d steps, final mass %.6f (base %.6f), N_TILT %.3g -> %.3f, tightened cone resolved to %.1e"
          % (len(g["run1_accepted"]), g["run1_x"][-1, 0], flight["x"][1, -1, 0], g["base_rep_1"][cr.IDX["N_TILT"]], g["run1_rep"][cr.IDX["N_TILT"]],
             abs(s1.min())))
    assert g["run1_accepted"].all() and g["run1_cnu"][-1] <= p.nuTol and g["run1_cdel"][-1] <= p.delTol
    assert s1.min() > -1e-6 and abs(s1.min()) == float(g["run1_viol"]) and g["run1_rep"][cr.IDX["N_TILT"]] >= 2.0
    assert g["run1_x"][-1, 0] < flight["x"][1, -1, 0]                # headroom costs propellant


# ---- the CPU twin ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    """tests/path_margin_port.cpp built with the flags of oracle/Makefile (the bitwise comparison with liboracle_port.so needs them)"""
    so = str(tmp_path_factory.mktemp("pm_port") / "libpath_margin_port.so")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-fopenmp", "-ffp-contract=off", "-std=c++17", "-shared", "-o", so,
                           os.path.join(ROOT, "tests", "path_margin_port.cpp"), "-lm"])
    return C.CDLL(so)


def _twin_socp(lib, p, it, ic, pm=None, marg=None, tol=1e-9, lin32=False):
    from oracle import port
    K = p.K
    NU = 5 if getattr(p, "fins", False) else 3
    c = port.consts(p, tol)
    a = [np.ascontiguousarray(v[None], float) for v in (it.x, it.u, it.endpoint, it.deriv)]
    rk, icv = np.array([it.rk], float), np.ascontiguousarray(ic, float)
    sol, nu, info = np.zeros((K + 1) * (14 + NU) + 1), np.zeros((K, 14)), np.zeros(4)
    ptr = lambda v: v.ctypes.data_as(_dp)   # noqa: E731
    keep = [None if v is None else np.ascontiguousarray(v, float) for v in (marg, pm)]
    rc = lib.path_margin_port_socp(C.byref(c), C.c_int(1), ptr(a[0]), ptr(a[1]), ptr(a[2]), ptr(a[3]), ptr(rk), ptr(icv), ptr(sol), ptr(nu), ptr(info),
                                   *(None if v is None else ptr(v) for v in keep), C.c_int(NU), C.c_int(int(lin32)))
    assert rc == 0
    nx = 14 * (K + 1)
    return dict(dx=sol[:nx].reshape(K + 1, 14), du=sol[nx:nx + NU * (K + 1)].reshape(K + 1, NU), ds=sol[-1], nu=nu, status=int(info[0]),
                iters=int(info[1]), merit=info[2], pobj=info[3])


@pytest.mark.parametrize("name", ["k9", "k50", "k50f", "fin", "k100"])
def test_twin_with_backoffs_against_the_independent_oracle(twin, name):
    """"k100": the largest twin-to-oracle distance over x, u, dsigma, nu and the three starts is d100, on which the device's bound at
    K = 100 rests (test_gpu_path_margins.py).  The device is held to the 2e-5 of the other groups if d100 <= 5e-6 (the twin is at
    4e-6 on the K = 50 groups); measured on the CPU: 1.04e-5 / 1.16e-6 / 2.98e-6 on starts 0 / 1 / 2 (all in x; u 6.7e-6, dsigma
    5.4e-8, nu 1.1e-9 at most; objective 1.9e-10 relative), so d100 = D100 = 1.0434e-5 > 5e-6 and the device's bound there is 4 D100.
    The twin itself stays within the 2e-5 of every group, and within D100, which is asserted so that D100 cannot go stale."""
    from oracle import scvx
    g = _fixture(name)
    p = _flyable({"k9": 9, "k100": 100}.get(name, 50), fins=name == "fin")
    K = p.K
    for t in range(3):
        ic, pm = g[name + "_ic"][t], g[name + "_pm"][t]
        it = scvx.create_initial(p, 10, ic[:3], ic[3:])
        r = _twin_socp(twin, p, it, ic, pm, lin32=name == "k50f")
        x, u = it.x + r["dx"], it.u + r["du"]
        ref = {k: g["%s_%s" % (name, k)][t] for k in ("x", "u", "dsig", "nu", "pobj")}
        ex, eu, es, en = (float(np.abs(x - ref["x"]).max()), float(np.abs(u - ref["u"]).max()), float(abs(r["ds"] - ref["dsig"])),
                          float(np.abs(r["nu"] - ref["nu"]).max()))
        obj = -x[K, 0] + p.wNu * np.linalg.norm(r["nu"]) + 0.5 * np.linalg.norm(np.concatenate([r["dx"].ravel(), r["du"].ravel()])) + abs(r["ds"])
        s = pr.slacks(p, x, pm)
        print("%s start %d: status %d merit %.2e its %d; twin-vs-oracle x %.2e u %.2e dsigma %.2e nu %.2e; objective %.10f vs %.10f; smallest "
              "tightened slacks %s" % (name, t, r["status"], r["merit"], r["iters"], ex, eu, es, en, obj, ref["pobj"], s.min(axis=0)))
        assert r["status"] == 0 and r["merit"] < 1e-9
        assert ex < 2e-5 and eu < 2e-5 and es < 2e-5 and en < 2e-5
        assert abs(obj - ref["pobj"]) < 1e-8 * abs(ref["pobj"])
        assert s.min() > -1e-8
        if name == "k100":
            print("k100 start %d: d100 = %.4e (objective: %.2e relative)" % (t, max(ex, eu, es, en), abs(obj - ref["pobj"]) / abs(ref["pobj"])))
            assert max(ex, eu, es, en) <= D100


def test_twin_without_backoffs_is_the_port_bit_for_bit(twin):
    from oracle import port, scvx
    g = _fixture()
    for name, p in (("k9", _flyable(9)), ("k50", _flyable())):
        ic = g[name + "_ic"][1]
        it = scvx.create_initial(p, 10, ic[:3], ic[3:])
        want = port.socp(p, it.x[None], it.u[None], it.endpoint[None], it.deriv[None], it.rk, ic[None], tol=1e-9, nthreads=1)
        for label, pm in (("null", None), ("zero", np.zeros((p.K + 1, 4)))):
            r = _twin_socp(twin, p, it, ic, pm)
            assert r["status"] == want["status"][0] == 0 and r["iters"] == want["iters"][0], (name, label)
            for k in ("dx", "du", "nu"):
                assert np.array_equal(r[k], want[k][0]), (name, label, k)
            assert r["ds"] == want["ds"][0] and r["merit"] == want["merit"][0] and r["pobj"] == want["pobj"][0], (name, label)
        # ... and the thrust back-offs alone are those of the port's own entry
        lo = np.full((p.K + 1, 2), 2e-3)
        wm = port.socp(p, it.x[None], it.u[None], it.endpoint[None], it.deriv[None], it.rk, ic[None], tol=1e-9, nthreads=1, marg=lo[None])
        r = _twin_socp(twin, p, it, ic, None, marg=lo)
        assert np.array_equal(r["dx"], wm["dx"][0]) and np.array_equal(r["du"], wm["du"][0]) and r["iters"] == wm["iters"][0]
        moved = float(np.abs(_twin_socp(twin, p, it, ic, g[name + "_pm"][1])["dx"] - want["dx"][0]).max())
        print("%s: bitwise without back-offs; with the fixture's the minimiser moves by %.3e" % (name, moved))
        assert moved > 1e-4
        assert twin.path_margin_port_work_doubles(C.c_int(p.K), C.c_int(3)) > 0
