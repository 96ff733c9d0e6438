"""Independent CPU reference of the segment audit and of the back-offs taken from it (scvx_segment_audit_f64,
scvx_batch_audit_margins, include/scvx.h) -- a helper module, not a test file.

The per-segment columns are a few numpy lines over the sample states of flight_reference.chain(..., PLAN), the chain the flight
check's reference is made of; the back-off rule is restated in numpy (accumulation, caps, forced zeros); the hardening loop drives
the independent oracle through path_margin_reference.solve from oracle.scvx.create_initial.  Nothing here reads the device.
"""
import numpy as np

import flight_reference as fr
import path_margin_reference as pr

SEG_N = 11
COLUMNS = ("DEFECT", "G_MASS", "G_GLIDE", "G_TILT", "G_RATE", "G_TMAX", "G_TMIN", "G_GIMBAL", "G_DP", "G_FIN", "QNORM")
IDX = {n: i for i, n in enumerate(COLUMNS)}
STATE_COLUMNS = ("DEFECT", "G_MASS", "G_GLIDE", "G_TILT", "G_RATE", "G_DP", "QNORM")   # NaN where the segment has a non-finite sample
KIND_COLUMN = {"thrust": "G_TMIN", "glide": "G_GLIDE", "tilt": "G_TILT", "rate": "G_RATE"}


def columns(p, x, S, US):
    """seg [B][K][11] from the sample states S [B][K][nsub+1][14] and controls US [B][K][nsub+1][nu] of a PLAN chain of the plans x;
    p: an oracle.model.DescentProblem (enforce_dp / fins select the optional columns)."""
    x = np.asarray(x, float)
    B, K = S.shape[:2]
    tggs = np.tan(np.radians(p.gammaGs))                       # oracle/socp.py:99
    sqcm = np.sqrt((1 - np.cos(np.radians(p.thetaMax))) / 2)   # :100
    delMax = np.cos(np.radians(p.deltaMax))                    # :101
    n = np.linalg.norm
    r = np.full((B, K, SEG_N), -np.inf)
    with np.errstate(all="ignore"):
        r[..., IDX["DEFECT"]] = np.abs(S[:, :, -1] - x[:, 1:]).max(axis=-1)
        r[..., IDX["G_MASS"]] = (p.mdry - S[..., 0]).max(axis=-1)
        r[..., IDX["G_GLIDE"]] = (tggs * n(S[..., 2:4], axis=-1) - S[..., 1]).max(axis=-1)
        r[..., IDX["G_TILT"]] = (n(S[..., 9:11], axis=-1) - sqcm).max(axis=-1)
        r[..., IDX["G_RATE"]] = (n(S[..., 11:14], axis=-1) - p.omMax).max(axis=-1)
        un = n(US[..., :3], axis=-1)
        r[..., IDX["G_TMAX"]] = (un - p.Tmax).max(axis=-1)
        r[..., IDX["G_TMIN"]] = (p.Tmin - un).max(axis=-1)
        r[..., IDX["G_GIMBAL"]] = (un - US[..., 0] / delMax).max(axis=-1)
        if getattr(p, "enforce_dp", False):
            r[..., IDX["G_DP"]] = (n(S[..., 4:7], axis=-1) - float(np.sqrt(2.0 * p.dpMax / p.rho))).max(axis=-1)   # :188
        if getattr(p, "fins", False):
            r[..., IDX["G_FIN"]] = (n(US[..., 3:5], axis=-1) - p.finmxf).max(axis=-1)
        r[..., IDX["QNORM"]] = np.abs(n(S[..., 7:11], axis=-1) - 1.0).max(axis=-1)
        bad = ~np.isfinite(S).all(axis=(2, 3))
    for name in STATE_COLUMNS:
        if name == "G_DP" and not getattr(p, "enforce_dp", False):
            continue
        r[bad, IDX[name]] = np.nan
    return r


def audit(dyn, p, x, u, sigma, nsub, par=None):
    """(seg [B][K][11], PLAN-mode flight report [B][16]) of the plans (x, u, sigma) under problem p"""
    par = par if par is not None else dyn.Params(p)
    S, US, xfly = fr.chain(dyn, par, x, u, sigma, nsub, fr.PLAN)
    return columns(p, x, S, US), fr.report(p, x, S, US, xfly)


def report_from_seg(seg):
    """the columns of the PLAN-mode report that are maxima of seg: {report column: [B]}"""
    out = {"GAP": seg[..., IDX["DEFECT"]].max(axis=1), "QNORM": seg[..., IDX["QNORM"]].max(axis=1)}
    out.update({n: seg[..., IDX[n]].max(axis=1) for n in COLUMNS if n.startswith("G_")})
    return out


def excess(seg_col, tol):
    """e [K+1] from one seg column [K]: per node the larger excess over tol of the two segments that meet there"""
    ex = np.where(seg_col > tol, seg_col, 0.0)
    return np.maximum(np.concatenate([[0.0], ex]), np.concatenate([ex, [0.0]]))


def backoff_rule(p, x, seg, lo, pm, kinds, gain, tol, cap):
    """(lo [K+1], pm [K+1][4]) after one scvx_batch_audit_margins on ONE plan: x [K+1][14] the iterate, seg [K][11] its audit, lo and pm
    what the batch carries (zeros for none).  new = min(old + gain e_k, cap width_k); the widths and forced zeros are those of
    path_margin_reference.margins_from_sigma / scvx_batch_margins_from_cov.  A NaN in a selected column leaves everything as it is."""
    K = p.K
    x, seg = np.asarray(x, float), np.asarray(seg, float)
    lo, pm = np.array(lo, float), np.array(pm, float)
    assert all(k in KIND_COLUMN for k in kinds) and len(kinds) > 0, kinds
    if any(np.isnan(seg[:, IDX[KIND_COLUMN[k]]]).any() for k in kinds):
        return lo, pm
    tggs, sqcm = pr.consts(p)
    width = {"glide": np.maximum(x[:, 1], 0.0) * (1.0 / tggs), "tilt": np.full(K + 1, sqcm), "rate": np.full(K + 1, p.omMax)}
    for k in kinds:
        e = excess(seg[:, IDX[KIND_COLUMN[k]]], tol)
        if k == "thrust":
            lo = np.minimum(lo + gain * e, cap * (p.Tmax - p.Tmin))
            continue
        c = pr.KINDS.index(k)
        pm[:, c] = np.minimum(pm[:, c] + gain * e, cap * width[k])
        pm[K, c] = 0.0
        if k in ("glide", "rate"):
            pm[0, c] = 0.0
    return lo, pm


def violations(seg, kinds, tol):
    """{kind: (number of segments with G > tol, the largest G)} of one plan's seg [K][11]"""
    return {k: (int((seg[:, IDX[KIND_COLUMN[k]]] > tol).sum()), float(seg[:, IDX[KIND_COLUMN[k]]].max())) for k in kinds}


def harden(p, ic, x, u, sigma, kinds, gain, tol, cap, nsub, rounds, solver_tol=1e-8):
    """The hardening loop on ONE plan through the independent oracle, FROM THE STRAIGHT-LINE GUESS every round (the oracle's own
    interior-point method does not survive a replan from the converged plan under these small, sparse back-offs).  (x, u, sigma): the
    base plan; ic [6].  Per round: the audit of the current plan, the back-off rule on top of what is carried, then
    path_margin_reference.solve from oracle.scvx.create_initial.  Stops when no selected G > tol.  Returns (base seg, list of
    dict(lo, pm, accepted, cnu, cdel, rk, x, u, sigma, seg) per round); raises RuntimeError when the oracle does not converge."""
    from oracle import dynamics as od, scvx
    K = p.K
    lo, pm = np.zeros(K + 1), np.zeros((K + 1, 4))
    seg = audit(od, p, x[None], u[None], np.array([sigma]), nsub)[0][0]
    base, out = seg, []
    for _ in range(rounds):
        if not any(v[0] for v in violations(seg, kinds, tol).values()):
            break
        lo, pm = backoff_rule(p, x, seg, lo, pm, kinds, gain, tol, cap)
        it, cnu, cdel, log = pr.solve(scvx.create_initial(p, nsub, ic[:3], ic[3:]), pm, lo, np.zeros(K + 1), tol=solver_tol)
        if not (cnu <= p.nuTol and cdel <= p.delTol):
            raise RuntimeError("imax reached at |nu| = %.3e, dJ = %.3e" % (cnu, cdel))
        x, u, sigma = it.x, it.u, float(it.sigma)
        seg = audit(od, p, x[None], u[None], np.array([sigma]), nsub)[0][0]
        out.append(dict(lo=lo.copy(), pm=pm.copy(), accepted=np.array([e["accepted"] for e in log], np.int8),
                        cnu=np.array([e["cnu"] for e in log]), cdel=np.array([e["cdel"] for e in log]),
                        rk=np.array([e["rk"] for e in log]), x=x, u=u, sigma=np.array(sigma), seg=seg))
    return base, out
