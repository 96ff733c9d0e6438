"""The method of the interior-point path comparison (tests/k4_path_reference.py, tests/test_gpu_k4_path.py), checked without a GPU on the
conic solver's CPU twin alone:

  * yardstick drift: the yardstick recomputed here agrees with tests/golden/k4_path_yardstick.npz within a factor of 3 (the native
    build differs from machine to machine: nothing tighter means anything), above an absolute 1e-15 (depth 1 sits on single
    roundings); iteration counts and statuses are identical between the twin's two builds for every case and depth, and equal the
    fixture's;
  * depth choice: at every truncated depth n a case keeps, the twin's merit is below the merit at every earlier depth by more than a
    relative 1e-6 -- the solver returns the BEST iterate, and a near-tie could be decided differently by the device.  (The best merit
    so far never rises, so "every earlier depth" is depth n - 1.)  A depth that fails is dropped in k4_path_reference.DROPPED_DEPTHS,
    here on the CPU and never on the GPU;
  * mutation: the twin with its Schur factor forced to float (SCVX_PORT_FAC32=1 against =0) on exo K = 50 exceeds 10 Y by a factor of
    more than 1000 at some depth <= 6 and stays below 1e-5 at full depth: the path bound sees what the end bounds do not;
  * thrust back-offs on the twin (port.socp(marg=)): zero back-offs reproduce the unmargined twin bit for bit, and the back-offs of
    tests/golden/oracle_margin_runs.npz meet its `sub_` record (the independent oracle's solve of the edited SOCP) at the bounds of
    tests/test_gpu_margins.py: 2e-5 on the minimiser and 1e-8 relative on the objective, both sides at 1e-9."""
import ctypes as C
import os

import numpy as np
import pytest

import k4_path_reference as kp
from conftest import GOLDEN

_MEASURED = {}


def _measure(case):
    if case not in _MEASURED:
        _MEASURED[case] = kp.measure(case)
    return _MEASURED[case]


@pytest.mark.parametrize("case", list(kp.CASES))
def test_yardstick_agrees_with_the_fixture_and_the_two_builds_take_the_same_path(case):
    g = np.load(kp.FIXTURE)
    assert tuple(g["depths"]) == kp.DEPTHS and tuple(g["groups"]) == kp.GROUPS and list(g["cases"]) == list(kp.CASES)
    m = _measure(case)
    k = kp.key(case)
    assert np.array_equal(m["iters"], m["native_iters"]) and np.array_equal(m["status"], m["native_status"])
    assert bool(g["counts_identical_" + k])
    assert np.array_equal(m["iters"], g["iters_" + k]) and np.array_equal(m["status"], g["status_" + k])
    Y, Yf = np.maximum(m["native"], m["perturb"]), kp.yardstick(case, g)
    # per group: the largest over the truncated depths, and the full depth (the rows of the table in tests/test_gpu_k4_path.py)
    rows = lambda a: np.stack([a[:-1].max(axis=0), a[-1]])   # noqa: E731
    ratio = np.maximum(rows(Y), 1e-15) / np.maximum(rows(Yf), 1e-15)
    print("%s: yardstick here / fixture between %.2f and %.2f; largest at depth <= 12 %s, full %s"
          % (case, ratio.min(), ratio.max(), " ".join("%.1e" % v for v in Y[:-1].max(axis=0)), " ".join("%.1e" % v for v in Y[-1])))
    assert ratio.max() <= 3.0 and ratio.min() >= 1.0 / 3.0, ratio


@pytest.mark.parametrize("case", list(kp.CASES))
def test_kept_depths_have_a_clear_best_iterate(case):
    import oracle
    oracle.use_native(False)
    po, ic, marg, xb, ub, sg, e, d = kp.cpu_inputs(case)
    merit = {n: kp.run_twin(case, po, ic, marg, xb, ub, e, d, n) for n in range(1, 13)}
    keep = merit[12]["status"] != 5
    tie = [n for n in range(2, 13) if not np.all(merit[n]["merit"][keep] < merit[n - 1]["merit"][keep] * (1.0 - 1e-6))]
    print("%s: depths without a clear best iterate %s; dropped %s" % (case, tie, kp.DROPPED_DEPTHS.get(case, ())))
    assert set(kp.DROPPED_DEPTHS.get(case, ())) == set(tie) & set(kp.DEPTHS)
    assert not set(kp.depths_of(case)) & set(tie)
    for n in kp.depths_of(case)[:-1]:    # a truncated solve stops at its depth unless it is done or infeasible before
        st, its = merit[n]["status"], merit[n]["iters"]
        assert np.all((st == 5) | ((st == 1) & (its == n)) | ((st == 0) & (its <= n))), (n, st, its)


def test_float_factor_mutation_shows_on_the_path_and_not_at_the_end(monkeypatch):
    import oracle
    from oracle import port, port_lib
    oracle.use_native(False)
    case = "exo K=50"
    po, ic, marg, xb, ub, sg, e, d = kp.cpu_inputs(case)
    B, K = ic.shape[0], po.K
    port_lib().scvx_port_work_doubles_nu.restype = C.c_size_t
    nw = port_lib().scvx_port_work_doubles_nu(C.c_int(K), C.c_int(0), C.c_int(3))
    Y = kp.yardstick(case)
    worst, res = 0.0, {}
    for i, n in enumerate(kp.DEPTHS):
        for fac in ("0", "1"):
            monkeypatch.setenv("SCVX_PORT_FAC32", fac)
            res[fac] = port.socp(po, xb, ub, e, d, 100.0, ic, max_iter=n, retries=0, work=np.zeros((B, nw)), warm=np.zeros(B, np.int32))
        dist = kp.distance(res["0"], res["1"])[:4]
        ratio = float((dist / (kp.FACTOR * Y[i, :4])).max())
        print("depth %2d: float factor against double factor dx %.1e du %.1e dsigma %.1e nu %.1e = %.1e x (10 Y); iterations %s / %s"
              % (n, dist[0], dist[1], dist[2], dist[3], ratio, res["0"]["iters"], res["1"]["iters"]))
        if n <= 6:
            worst = max(worst, ratio)
    assert worst > 1000.0, worst
    assert dist.max() < 1e-5, dist       # ... and at full depth the two are as close as today's end bounds allow
    assert np.all(res["0"]["status"] == 0) and np.all(res["1"]["status"] == 0)


def test_zero_backoffs_reproduce_the_unmargined_twin_bit_for_bit():
    import oracle
    from oracle import port
    oracle.use_native(False)
    for case, lin32 in (("thrust back-offs", False), ("exo K=9", False), ("float tiles", True), ("fins K=9", False)):
        po, ic, marg, xb, ub, sg, e, d = kp.cpu_inputs(case)
        z = np.zeros((ic.shape[0], po.K + 1, 2))
        for n in (3, kp.FULL):
            a = port.socp(po, xb, ub, e, d, 100.0, ic, max_iter=n, retries=0, lin32=lin32)
            b = port.socp(po, xb, ub, e, d, 100.0, ic, max_iter=n, retries=0, lin32=lin32, marg=z)
            for k in a:
                assert np.array_equal(a[k], b[k]), (case, n, k)
    # ... and back-offs that bind move the solve
    po, ic, marg, xb, ub, sg, e, d = kp.cpu_inputs("thrust back-offs")
    a = port.socp(po, xb, ub, e, d, 100.0, ic, retries=0)
    b = port.socp(po, xb, ub, e, d, 100.0, ic, retries=0, marg=marg)
    assert np.abs(a["du"] - b["du"]).max() > 1e-4


def test_fixture_backoffs_on_the_twin_meet_the_independent_oracle():
    import oracle
    from oracle import port
    oracle.use_native(False)
    g = np.load(os.path.join(GOLDEN, "oracle_margin_runs.npz"))
    po, ic, marg, xb, ub, sg, e, d = kp.cpu_inputs("thrust back-offs")
    K = po.K
    tw = port.socp(po, xb, ub, e, d, 100.0, ic, tol=1e-9, marg=marg)
    x, u = xb + tw["dx"], ub + tw["du"]
    ex, eu, es, en = (float(np.abs(x - g["sub_x"]).max()), float(np.abs(u - g["sub_u"]).max()), float(np.abs(tw["ds"] - g["sub_dsig"]).max()),
                      float(np.abs(tw["nu"] - g["sub_nu"]).max()))
    obj = (-x[0, K, 0] + po.wNu * np.linalg.norm(tw["nu"][0]) + 0.5 * np.linalg.norm(np.concatenate([tw["dx"][0].ravel(), tw["du"][0].ravel()]))
           + abs(tw["ds"][0]))
    t = np.linalg.norm(u[0, :, :3], axis=1)
    print("twin under the fixture's back-offs: status %s merit %.2e its %s; twin-vs-oracle x %.2e u %.2e dsigma %.2e nu %.2e; objective %.10f vs %.10f; "
          "Tmax - hi - |u| >= %.2e" % (tw["status"], tw["merit"][0], tw["iters"], ex, eu, es, en, obj, g["sub_pobj"][0], (po.Tmax - marg[0, :, 1] - t).min()))
    assert tw["status"][0] == 0 and tw["merit"][0] < 1e-9
    assert ex < 2e-5 and eu < 2e-5 and es < 2e-5 and en < 2e-5
    assert abs(obj - g["sub_pobj"][0]) < 1e-8 * abs(g["sub_pobj"][0])
    assert (t <= po.Tmax - marg[0, :, 1] + 1e-8).all()
