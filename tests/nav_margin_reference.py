"""Independent CPU reference of the back-offs taken from the navigation analysis (scvx_nav_path_sigma_f64 /
scvx_batch_margins_from_nav, include/scvx.h) -- a helper module, not a test file.

Nothing new is computed here: the per-node standard deviations are margin_reference.path_sigma (gradients: cov_reference.path_grad)
on the TRUTH block Xi_k[z, z] of nav_reference.propagate's joint covariance, before the update at the node -- the constraints bind the
vehicle, not its estimate.  The conic solves under back-offs are margin_reference's.  Nothing here reads the device.
"""
import math

import numpy as np

import margin_reference as mr
import nav_reference as nr

THRUST = mr.PSIG_COLUMNS.index("THRUST")


def position_model(x0):
    """(H, rm) of the checks: POSITION ONLY measured at every node, the position rows of test_nav_cpu.pv_model (1 sigma = 3e-5 of the
    largest |r| component of x0)"""
    from successiveconvexification_amd.montecarlo import measurement_rows
    from test_nav_cpu import pv_model
    return measurement_rows("r"), pv_model(x0)[1][:3].copy()


def path_sigma(p, x, u, deriv, K, gain, S0, N0, H=None, rm=None, w=None, dtype=np.float64):
    """psig [B][K+1][5] in `dtype` of the closed loop flown on an estimate.  Node 0 is 0; a node whose gradient is undefined is 0; a
    trajectory with a non-finite entry anywhere in its joint covariance (either block: the device's two flags) is NaN."""
    joint, _, _ = nr.propagate(deriv, K, gain, S0, N0, H, rm, w, dtype)
    n = joint.shape[-1] - 14
    ps = mr.path_sigma(p, x, u, joint[:, :, :n, :n], dtype)
    for b in range(joint.shape[0]):
        if not np.isfinite(joint[b].astype(np.float64)).all():
            ps[b] = np.nan
    return ps


def variance_yardstick(p, x, u, E):
    """[B][K+1][5]: how far c' Sigma c may move when every entry of Sigma moves by at most E[b]: |c|_1^2 E[b] with the gradients of
    cov_reference.path_grad (0 at node 0 and where the gradient is undefined) -- the rounding yardstick of a VARIANCE; a standard
    deviation s moves by that over 2 s, which is why small s are compared as variances"""
    import cov_reference as cr
    x, u = np.asarray(x, float), np.asarray(u, float)
    out = np.zeros(x.shape[:2] + (5,))
    for b in range(x.shape[0]):
        for k in range(1, x.shape[1]):
            c = cr.path_grad(p, x[b, k], u[b, k])[:5]
            l1 = np.abs(c).sum(axis=1)
            out[b, k] = np.where(np.isnan(l1), 0.0, l1 * l1) * E[b]
    return out


def backoffs(p, psig, nsigma=3.0, cap=0.25):
    """lo = hi [..][K+1] of the thrust band: min(nsigma s_T(k), cap (Tmax - Tmin))"""
    return np.minimum(nsigma * np.asarray(psig, float)[..., THRUST], cap * (p.Tmax - p.Tmin))


def outside_band(p, u, psig, flights=256):
    """First-order expected number of node controls commanded outside [Tmin, Tmax] over `flights` closed loops of ONE plan u [K+1][nu]:
    |u_k| is Gaussian about the plan's with standard deviation psig[k][THRUST], so node k contributes
    flights (Phi(-(|u_k| - Tmin) / s) + Phi(-(Tmax - |u_k|) / s)); a node with s = 0 contributes nothing unless the plan is outside."""
    t = np.linalg.norm(np.asarray(u, float)[:, :3], axis=-1)
    s = np.asarray(psig, float)[:, THRUST]
    tot = 0.0
    for k in range(1, t.shape[0]):
        for gap in (t[k] - p.Tmin, p.Tmax - t[k]):
            if s[k] > 0.0:
                tot += 0.5 * math.erfc(gap / s[k] / math.sqrt(2.0))
            elif gap < 0.0:
                tot += 1.0
    return flights * tot
