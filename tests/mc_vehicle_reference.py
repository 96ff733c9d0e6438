"""Independent CPU reference of the sampled closed-loop dispersion with per-flight VEHICLE ERRORS (the _veh forms, include/scvx.h) -- a
helper module, not a test file.

It is mc_reference.chain with two controls kept apart: the law, the clamp, the counters and the report see the COMMANDED control, the
integrator (flight_reference._substeps: the C oracle, or aero_torque_reference for the torque models) is fed the APPLIED one,
    ua[0:3] = (1 + th0) (u[0:3] + d x u[0:3]),  d = (0, th1, th2);      ua[3:5] = (1 + th5) u[3:5]
formed at the two ends of every segment's hold -- the map is linear in u, so applying it to the ends of a first-order hold is applying
it at every stage.  alpha (1 + th3) and force_scalar (1 + th4) are not patched into the integrator: each distinct (th3, th4) gets a
parameter set of its own, built by the integrator's own constructor from a problem with the scaled constants (the torque model's
trq_scalar = length_scalar * force_scalar follows force_scalar there).  Flights are grouped by their (th3, th4): one group when those
two are not dispersed, one flight per group when they are.
"""
from dataclasses import replace

import numpy as np

import flight_reference as fr
import track_reference as tr

N = 6
THRUST, MIS_Y, MIS_Z, ISP, AERO, FIN = range(N)


def apply(u, th):
    """the applied control of the commanded u [F][nu] under th [F][6]"""
    u, th = np.asarray(u, float), np.asarray(th, float)
    ua = np.empty_like(u)
    sc = 1.0 + th[:, THRUST]
    ua[:, 0] = sc * (u[:, 0] + (th[:, MIS_Y] * u[:, 2] - th[:, MIS_Z] * u[:, 1]))
    ua[:, 1] = sc * (u[:, 1] + th[:, MIS_Z] * u[:, 0])
    ua[:, 2] = sc * (u[:, 2] - th[:, MIS_Y] * u[:, 0])
    if u.shape[1] == 5:
        ua[:, 3:5] = (1.0 + th[:, FIN])[:, None] * u[:, 3:5]
    return ua


def scaled_params(dyn, p, par, th3, th4):
    """the integrator's parameter set of the problem p with alpha (1 + th3) and force_scalar (1 + th4); par itself for (0, 0)"""
    if th3 == 0.0 and th4 == 0.0:
        return par
    q = replace(p, alpha=p.alpha * (1.0 + th3))
    if th4 != 0.0:
        if p.aero is None:
            raise ValueError("AERO on a model without aerodynamics")
        q = replace(q, aero=replace(p.aero, force_scalar=p.aero.force_scalar * (1.0 + th4)))
    return dyn.Params(q, torque=True) if getattr(par, "torque", False) else dyn.Params(q)


def chain(dyn, par, p, x, u, sigma, gain, dx0, nsub, theta, flags=0, imp=None, nav=None):
    """mc_reference.chain with vehicle errors theta [F][6]: (samples, their COMMANDED controls, xfly, ufly -- commanded --, commanded
    thrust norms before the clamp [F][K]).  nav [F][K][14] = eps+_k: the law is fed the estimate, as mc_nav_reference.chain feeds it"""
    x, u, sigma, theta = np.asarray(x, float), np.asarray(u, float), np.asarray(sigma, float), np.asarray(theta, float)
    B, K1, _ = x.shape
    K = K1 - 1
    dt = 1.0 / (K + 1)
    nu = u.shape[-1]
    if nu != 5 and theta[:, FIN].any():
        raise ValueError("FIN on a model without fins")
    keys = {}
    for f in range(B):
        keys.setdefault((float(theta[f, ISP]), float(theta[f, AERO])), []).append(f)
    groups = [(np.array(rows), scaled_params(dyn, p, par, *k)) for k, rows in keys.items()]
    lam = np.arange(nsub + 1) / nsub
    S, US = np.empty((B, K, nsub + 1, 14)), np.empty((B, K, nsub + 1, nu))
    xfly, ufly = np.empty((B, K1, 14)), np.empty((B, K1, nu))
    cmd = np.empty((B, K))
    cur = x[:, 0].copy() if dx0 is None else x[:, 0] + np.asarray(dx0, float)
    xfly[:, 0] = cur
    ufly[:, 0] = u[:, 0]
    with np.errstate(all="ignore"):
        for k in range(K):
            fed = cur if nav is None else cur - np.asarray(nav, float)[:, k]
            z = np.concatenate([fed - x[:, k], ufly[:, k] - u[:, k]], axis=1)
            un = u[:, k + 1] + np.einsum("bji,bi->bj", np.asarray(gain, float)[:, k], z)
            cmd[:, k] = np.linalg.norm(un[:, :3], axis=1)
            if flags & tr.CLAMP:
                un = tr.clamp_control(p, un)
            ufly[:, k + 1] = un
            a0, a1 = apply(ufly[:, k], theta), apply(ufly[:, k + 1], theta)
            for rows, pr in groups:
                S[rows, k], _ = fr._substeps(dyn, pr, cur[rows], a0[rows], a1[rows], sigma[rows], dt, nsub)
            # the commanded hold at the samples, by flight_reference._substeps' own expression
            US[:, k] = ufly[:, k, None, :] * (1.0 - lam)[None, :, None] + ufly[:, k + 1, None, :] * lam[None, :, None]
            cur = S[:, k, -1] if imp is None else S[:, k, -1] + imp[:, k]
            xfly[:, k + 1] = cur
    return S, US, xfly, ufly, cmd


def fly_plan(dyn, p, xb, ub, sb, gb, dx0, nsub, theta, flags=0, imp=None, par=None, nav=None):
    """(flights [F][16], xfly, ufly, commanded thrust norms [F][K]) of F flights of ONE plan, flight f with theta[f]"""
    par = par if par is not None else dyn.Params(p)
    F = np.shape(theta)[0]
    bc = lambda a: np.broadcast_to(np.asarray(a, float), (F,) + np.shape(a))   # noqa: E731
    d0 = np.zeros((F, 14)) if dx0 is None else dx0
    S, US, xfly, ufly, cmd = chain(dyn, par, p, bc(xb), bc(ub), np.full(F, float(sb)), bc(gb), d0, nsub, theta, flags, imp, nav)
    return fr.report(p, bc(xb), S, US, xfly), xfly, ufly, cmd


def sensitivity_fd(dyn, p, xb, ub, sb, gb, nsub, h, comps, flags=0, par=None):
    """J [14][6] = d x_K / d theta about theta = 0 and the planned start by central differences of step h through the chain; the columns
    outside `comps` are zero"""
    th = np.zeros((2 * len(comps), N))
    for i, c in enumerate(comps):
        th[2 * i, c], th[2 * i + 1, c] = h, -h
    _, xf, _, _ = fly_plan(dyn, p, xb, ub, sb, gb, None, nsub, th, flags, None, par)
    J = np.zeros((14, N))
    for i, c in enumerate(comps):
        J[:, c] = (xf[2 * i, -1] - xf[2 * i + 1, -1]) / (2.0 * h)
    return J


def equal_share_sp(J, comps, trace0):
    """one sp for the components `comps` at which J diag(sp^2) J' has the trace trace0"""
    return float(np.sqrt(trace0 / sum(float(J[:, c] @ J[:, c]) for c in comps)))


def sensitivity(dyn, p, xb, ub, sb, gb, dx0, nsub, theta, eps, flags=0, imp=None, draws=3, seed=0, par=None, nav=None):
    """A_cl of the chain with vehicle errors, measured like mc_reference.sensitivity: starts perturbed by eps * xi scaled by the start's
    own components; largest deviation of any node state / largest initial perturbation, floored at 1"""
    par = par if par is not None else dyn.Params(p)
    d0 = np.asarray(dx0, float)
    rng = np.random.default_rng(seed)
    _, xf0, _, _ = fly_plan(dyn, p, xb, ub, sb, gb, d0, nsub, theta, flags, imp, par, nav)
    A = 1.0
    for _ in range(draws):
        pert = (np.asarray(xb, float)[0] + d0) * (eps * rng.uniform(-1.0, 1.0, d0.shape))
        _, xf, _, _ = fly_plan(dyn, p, xb, ub, sb, gb, d0 + pert, nsub, theta, flags, imp, par, nav)
        dev = np.abs(xf - xf0).max(axis=(1, 2))
        A = max(A, float((dev / np.abs(pert).max(axis=1)).max()))
    return A


def fma(a, b, c):
    """fma(a, b, c) entry by entry, correctly rounded: exact rational arithmetic, one rounding"""
    from fractions import Fraction
    a, b, c = np.broadcast_arrays(np.asarray(a, float), np.asarray(b, float), np.asarray(c, float))
    out = np.empty(a.shape)
    for i in np.ndindex(a.shape):
        out[i] = float(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
    return out
