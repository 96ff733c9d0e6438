"""The aerodynamic body torque (SCVX_MODEL_AERO_TORQUE, include/scvx.h) on the MI355X: K1 / K2 in every kernel form the flag routes to
against the independent torch reference (tests/aero_torque_reference.py: automatic differentiation of the segment map), the fp32 forms,
the ABI's argument checks, and full configs[2] / aero + fins runs against the oracle loop on the torque discretisation
(tests/golden/make_oracle_torque_runs.py)."""
import ctypes as C
import os
from dataclasses import replace

import numpy as np
import pytest

from conftest import GOLDEN, random_segments

pytestmark = pytest.mark.gpu

# test_golden_fixtures.AERO8_BOUNDS, restated: L-inf distance of the device iterate to the oracle's at every step
AERO8_BOUNDS = dict(mrv=5e-5, att=2e-3, u=5e-4, sigma=2e-4)


def _problems(fins, aero_tables, torque=True):
    from oracle import model
    from successiveconvexification_amd import sample_problems as sp
    from successiveconvexification_amd.defns import AtmosphericData
    a = AtmosphericData(*aero_tables)
    oa = model.AeroData(*aero_tables)
    if fins:
        return sp.base_prob_fin_scaled(a, torque=torque), model.base_prob_fin_scaled(oa)
    return sp.base_prob_aero_scaled(a, torque=torque), model.base_prob_scaled(oa)


def _segments(po, B, K, seed):
    x, u, sigma = random_segments(po, B, K, seed)
    if po.fins:
        u = np.concatenate([u, po.finmxf * np.random.default_rng(seed + 1).uniform(-0.7, 0.7, (B, K + 1, 2))], axis=-1)
    return x, u, sigma


ENVS = [{}, {"SCVX_K1_VARIANT": "0"}, {"SCVX_K1_SG": "0"}, {"SCVX_K1_PERSIST": "0"}, {"SCVX_K1_PERSIST": "1"}]
_REF = {}


def _reference(fins, B, K, npts, aero_tables):
    """segments and the AD reference's K1 result, once per shape (shared by the kernel-form variants)"""
    import aero_torque_reference as ref
    key = (fins, B, K, npts)
    if key not in _REF:
        po = _problems(fins, aero_tables)[1]
        x, u, sigma = _segments(po, B, K, 20261012 + B)
        _REF[key] = (x, u, sigma) + ref.linearize(ref.Params(po, torque=True), x, u, sigma, 1.0 / (K + 1), npts)
    return _REF[key]


@pytest.mark.parametrize("env", ENVS, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()) or "default")
@pytest.mark.parametrize("B,K,npts", [(16, 50, 10), (5, 100, 3), (2, 13, 1), (3, 1, 2)])
@pytest.mark.parametrize("fins", [False, True], ids=["aero", "aero+fins"])
def test_torque_linearize_and_propagate_match_the_reference(fins, B, K, npts, env, aero_tables, monkeypatch):
    """K1 (split producer from 3 substeps, else the stage-granular pipeline; the column-per-lane variant falls through to it) and K2 with
    the torque against the AD reference: endpoint 1e-12, derivative 1e-11 relative.  The torque must show in the rate rows."""
    from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch, propagate_batch
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    pp = _problems(fins, aero_tables)[0]
    x, u, sigma, e_ref, d_ref = _reference(fins, B, K, npts, aero_tables)
    dt = 1.0 / (K + 1)
    c = IntegratorCache(pp, npts=npts)
    e, d = linearize_batch(c, x, u, sigma, dt)
    scale = max(1.0, np.abs(d_ref).max())
    assert np.abs(e - e_ref).max() < 1e-12, np.abs(e - e_ref).max()
    assert np.abs(d - d_ref).max() < 1e-11 * scale, (np.abs(d - d_ref).max(), scale)
    xn = propagate_batch(c, x, u, sigma, dt)
    assert np.abs(xn - e_ref).max() < 1e-12 and np.abs(xn - e).max() < 1e-13
    c.close()
    # the same segments without the torque: the rate rows move by far more than the tolerance
    c0 = IntegratorCache(_problems(fins, aero_tables, torque=False)[0], npts=npts)
    e0, d0 = linearize_batch(c0, x, u, sigma, dt)
    assert np.abs(d - d0)[..., 11:14].max() > 1e-5 and np.abs(e - e0)[..., 11:14].max() > 1e-7
    c0.close()


def test_torque_first_order_taylor_property(aero_tables):
    """At the full batch (B = 8192): K2 finite differences against K1's derivative, second-order remainder only."""
    from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch, propagate_batch
    pp, po = _problems(False, aero_tables)
    B, K = 8192, 50
    x, u, sigma = random_segments(po, B, K, 20261004)
    dt = 1.0 / (K + 1)
    c = IntegratorCache(pp, npts=4)
    e, d = linearize_batch(c, x, u, sigma, dt)
    rng = np.random.default_rng(1)
    eps = 1e-6
    dx, du, ds = rng.normal(size=x.shape) * eps, rng.normal(size=u.shape) * eps, rng.normal(size=sigma.shape) * eps
    e2 = propagate_batch(c, x + dx, u + du, sigma + ds, dt)
    delta = np.concatenate([dx[:, :-1], du[:, :-1], du[:, 1:], np.broadcast_to(ds[:, None, None], (B, K, 1))], axis=-1)
    pred = np.einsum("bkji,bkj->bki", d, delta)
    err = np.abs(e2 - e - pred).max()
    assert err < 50 * eps * eps * 1e3, err
    c.close()


@pytest.mark.parametrize("fins", [False, True], ids=["aero", "aero+fins"])
def test_torque_fp32_forms(fins, aero_tables):
    """scvx_linearize_f32 / scvx_propagate_f32 and the float derivative tiles (scvx_batch_set_linearization_f32) with the torque, against
    the fp64 result: the stated 2e-5 (endpoint) / 2e-4 (derivative) relative."""
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch, linearize_batch_f32, propagate_batch_f32
    pp, po = _problems(fins, aero_tables)
    for npts in (2, 10):
        B, K = 12, 50
        x, u, sigma = _segments(po, B, K, 77 + npts)
        dt = 1.0 / (K + 1)
        c = IntegratorCache(pp, npts=npts)
        e64, d64 = linearize_batch(c, x, u, sigma, dt)
        e, d = linearize_batch_f32(c, x, u, sigma, dt)
        assert np.abs(e - e64).max() < 2e-5 * max(1.0, np.abs(e64).max())
        assert np.abs(d - d64).max() < 2e-4 * max(1.0, np.abs(d64).max())
        assert np.abs(propagate_batch_f32(c, x, u, sigma, dt) - e64).max() < 2e-5 * max(1.0, np.abs(e64).max())
        c.close()
    c = IntegratorCache(pp, npts=10)
    b = ScvxBatch(c, 8).init(None)
    e64, d64 = b.linearization()
    b.set_linearization_f32(True)
    e32, d32 = b.linearization()
    assert np.array_equal(e32, e64)                                 # the endpoint stays double
    assert np.abs(d32 - d64).max() <= 1e-6 * max(1.0, np.abs(d64).max())   # rounded once, at the store
    assert np.abs(d32 - d64).max() > 0.0
    b.close(); c.close()


def test_torque_argument_errors(aero_tables):
    from successiveconvexification_amd import _lib, sample_problems as sp
    from successiveconvexification_amd.defns import AtmosphericData
    L = _lib.lib()
    a = AtmosphericData(*aero_tables)

    def create(p):
        cp = p.to_c()
        h = C.c_void_p()
        rc = L.scvx_ctx_create(C.byref(cp), 0, C.byref(h))
        return rc, h

    rc, h = create(replace(sp.base_prob_scaled, model_flags=4))
    assert rc == -1 and not h.value                                  # the torque with ExoatmosphericData
    rc, h = create(replace(sp.base_prob_aero_scaled(a), model_flags=8))
    assert rc == -1 and not h.value                                  # a bit the library does not know
    d = np.ascontiguousarray(aero_tables[0], float)
    l = np.ascontiguousarray(aero_tables[1], float)
    nm, na = d.shape
    P = C.POINTER(C.c_double)
    for torque, want in ((True, -1), (False, 0)):
        rc, h = create(sp.base_prob_aero_scaled(a, torque=torque))
        assert rc == 0
        got = L.scvx_set_aero_table(h, d.ctypes.data_as(P), l.ctypes.data_as(P), None, na, nm, a.aoa0, a.daoa, a.mach0, a.dmach)
        assert got == want, (torque, got)
        L.scvx_ctx_destroy(h)


def _full_run(pp, ic, g, idx):
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache
    log = g["log"]
    c = IntegratorCache(pp, npts=10)
    b = ScvxBatch(c, ic.shape[0]).init(ic)
    worst = dict(mrv=0.0, att=0.0, u=0.0, sigma=0.0)
    for n in range(log.shape[1]):
        st, nun, dj = b.solve_step()
        assert np.isin(st, (0, 1, 2)).all(), (n, np.unique(st))
        x, u, s = b.trajectory()
        rk, cost, it = b.scalars()
        assert np.array_equal(rk[idx], log[:, n, 3]), (n, rk[idx], log[:, n, 3])
        d = np.abs(x[idx] - g["xs"][:, n])
        err = dict(mrv=d[..., :7].max(), att=d[..., 7:].max(), u=np.abs(u[idx] - g["us"][:, n]).max(),
                   sigma=np.abs(s[idx] - log[:, n, 5]).max())
        for k in worst:
            worst[k] = max(worst[k], err[k])
    b.close(); c.close()
    return worst


def test_torque_configs2_B256_full_run_matches_the_oracle_loop(aero_tables):
    """BASELINE configs[2] with the torque: B = 256 dispersed, all 14 solve_steps on the device; four trajectories against the oracle's
    loop on the torque discretisation at EVERY step (radius schedule exact, iterates within AERO8_BOUNDS)."""
    import bench
    pp, _ = _problems(False, aero_tables)
    g = np.load(os.path.join(GOLDEN, "oracle_scvx_aero_torque_batch4_tol1e-08.npz"))
    idx = g["index"]
    ic = bench.disperse_ics(pp, 0, 256, 20261003)
    assert np.array_equal(ic[idx], g["ic"])
    worst = _full_run(pp, ic, g, idx)
    print("device vs oracle loop, configs[2] + torque, worst over 14 steps:", {k: "%.2e" % v for k, v in worst.items()})
    for k, bd in AERO8_BOUNDS.items():
        assert worst[k] < bd, (k, worst[k])


def test_torque_aerofin_full_run_matches_the_oracle_loop(aero_tables):
    pp, _ = _problems(True, aero_tables)
    g = np.load(os.path.join(GOLDEN, "oracle_scvx_aerofin_torque_tol1e-08.npz"))
    worst = _full_run(pp, g["ic"], g, np.array([0]))
    print("device vs oracle loop, aero + fins + torque, worst over 14 steps:", {k: "%.2e" % v for k, v in worst.items()})
    for k, bd in AERO8_BOUNDS.items():
        assert worst[k] < bd, (k, worst[k])
