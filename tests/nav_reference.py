"""Independent CPU reference of the navigation-error (LQG) covariance analysis (scvx_nav_cov_f64 / scvx_track_fly_nav_f64,
include/scvx.h) -- a helper module, not a test file.

The recursion of the header on the joint zeta_k = [z_k; eps_k] in numpy with the FULL matrices T_k, U_k and Xi_k (the device kernel
never forms T or U: it uses their blocks; this does not), with a `dtype` argument: float64, or longdouble as the yardstick of the
float64 rounding error.  numpy.linalg refuses longdouble, so the solve with S is track_reference's hand-written Cholesky.  The
dispersion report comes from cov_reference.report on the z block; the navigation report is a few traces.  The gains are an
argument: the tests feed track_reference.gains, never the device's.

Closed loop: track_reference.chain with the navigation error injected into the law, z = [(x_fly - nav) - xbar; u - ubar]; the
integrator between the nodes is flight_reference._substeps (the C oracle), not restated.
"""
import numpy as np

import cov_reference as cr
import flight_reference as fr
import track_reference as tr

NAV_NREP = 8
NAV_COLUMNS = ("NAV_M", "NAV_R", "NAV_V", "NAV_Q", "NAV_W", "NAV_PEAK", "EST_R", "EST_V")
NAV_IDX = {n: i for i, n in enumerate(NAV_COLUMNS)}
BLOCKS = {"m": slice(0, 1), "r": slice(1, 4), "v": slice(4, 7), "q": slice(7, 11), "w": slice(11, 14)}


def propagate(deriv, K, gain, S0, N0, H=None, rm=None, w=None, dtype=np.float64):
    """(joint [B][K+1][N][N]: every pre-update Xi_k, kf [B][K][14][m], the largest cond(S_k) per trajectory [B]) in `dtype`"""
    A, Bm, Bp = tr.split_tiles(deriv, K)
    B, nu = A.shape[0], Bm.shape[-1]
    n = 14 + nu
    N = n + 14
    S0, N0 = cr.s0_full(S0, B), cr.s0_full(N0, B)
    m = 0 if H is None else np.asarray(H).shape[0]
    if m:
        Hm = np.asarray(H).astype(dtype).reshape(m, 14)
        R = np.diag(np.asarray(rm).astype(dtype))
    W = np.zeros((N, N), dtype)
    if w is not None:
        wv = np.broadcast_to(np.asarray(w), (14,)).astype(dtype)
        i = np.arange(14)
        W[i, i] = W[i, n + i] = W[n + i, i] = W[n + i, n + i] = wv
    joint = np.zeros((B, K + 1, N, N), dtype)
    kf = np.zeros((B, K, 14, m), dtype)
    cond = np.ones(B)
    for b in range(B):
        X = np.zeros((N, N), dtype)
        s0, n0 = S0[b].astype(dtype), N0[b].astype(dtype)
        X[:14, :14] = (s0 + s0.T) / 2
        X[n:, n:] = (n0 + n0.T) / 2
        joint[b, 0] = X
        for k in range(K):
            if m:
                P = X[n:, n:]
                S = Hm @ P @ Hm.T + R
                with np.errstate(all="ignore"):
                    sf = S.astype(np.float64)
                    if np.isfinite(sf).all():
                        cond[b] = max(cond[b], float(np.linalg.cond(sf)))
                Kf = tr._chol_solve(S, Hm @ P).T              # P H' S^-1 (P and S symmetric)
                U = np.eye(N, dtype=dtype)
                U[n:, n:] -= Kf @ Hm
                X = U @ X @ U.T
                X[n:, n:] += Kf @ R @ Kf.T
                kf[b, k] = Kf
            Ak = A[b, k].astype(dtype)
            F, G = tr.fg(Ak, Bm[b, k].astype(dtype), Bp[b, k].astype(dtype), dtype)
            L = np.asarray(gain[b, k]).astype(dtype)
            T = np.zeros((N, N), dtype)
            T[:n, :n] = F + G @ L
            T[:n, n:] = -(G @ L[:, :14])
            T[n:, n:] = Ak
            Y = T @ X @ T.T
            X = (Y + Y.T) / 2 + W
            joint[b, k + 1] = X
    return joint, kf, cond


def _sdv(d):
    """elementwise square root of variances: negative rounding residue is 0, a NaN stays a NaN"""
    return np.where(d > 0, np.sqrt(np.where(d > 0, d, 0)), np.where(d != d, d, 0))


def nav_report(joint, n, dtype=np.float64):
    """navrep [B][8] in `dtype` from every pre-update Xi_k"""
    joint = np.asarray(joint, dtype)
    B = joint.shape[0]
    out = np.zeros((B, NAV_NREP), dtype)
    for b in range(B):
        XK = joint[b, -1]
        P = XK[n:, n:]
        d = np.diag(P)
        for name, key in (("NAV_M", "m"), ("NAV_R", "r"), ("NAV_V", "v"), ("NAV_Q", "q"), ("NAV_W", "w")):
            out[b, NAV_IDX[name]] = cr._sd(d[BLOCKS[key]].sum())
        out[b, NAV_IDX["NAV_PEAK"]] = max(cr._sd(np.trace(joint[b, k, n:, n:])) for k in range(joint.shape[1]))
        C = XK[:14, n:]
        E = XK[:14, :14] - C - C.T + P                       # Cov(xhat_K - xbar_K)
        e = np.diag(E)
        out[b, NAV_IDX["EST_R"]] = cr._sd(e[BLOCKS["r"]].sum())
        out[b, NAV_IDX["EST_V"]] = cr._sd(e[BLOCKS["v"]].sum())
        if not np.isfinite(joint[b].astype(np.float64)).all():
            out[b] = np.nan
    return out


def run(p, x, u, deriv, K, gain, S0, N0, H=None, rm=None, w=None, dtype=np.float64, detail=False):
    """dict of report [B][16], navrep [B][8], joint, sig [B][K+1][n], navsig [B][K+1][14], kf, cond [B] (and the margins' detail)"""
    joint, kf, cond = propagate(deriv, K, gain, S0, N0, H, rm, w, dtype)
    n = joint.shape[-1] - 14
    rep = cr.report(p, x, u, joint[:, :, :n, :n], dtype, detail=detail)
    det = None
    if detail:
        rep, det = rep
    for b in range(joint.shape[0]):
        if not np.isfinite(joint[b].astype(np.float64)).all():
            rep[b] = np.nan
    d = np.diagonal(joint, axis1=-2, axis2=-1)
    return dict(report=rep, navrep=nav_report(joint, n, dtype), joint=joint, sig=_sdv(d[..., :n]), navsig=_sdv(d[..., n:]), kf=kf,
                cond=cond, detail=det)


# ---- the closed loop with the law fed an estimate, and the sampled check on the joint ----------------------------------------------
def chain(dyn, par, p, x, u, sigma, gain, dx0, nav, nsub):
    """track_reference.chain with the law fed the estimate: z = [(x_fly - nav_k) - xbar_k; u_k - ubar_k].  (xfly, ufly)"""
    x, u, sigma = np.asarray(x, float), np.asarray(u, float), np.asarray(sigma, float)
    B, K1, _ = x.shape
    K = K1 - 1
    dt = 1.0 / (K + 1)
    nu = u.shape[-1]
    xfly, ufly = np.empty((B, K1, 14)), np.empty((B, K1, nu))
    cur = x[:, 0].copy() if dx0 is None else x[:, 0] + np.asarray(dx0, float)
    xfly[:, 0] = cur
    ufly[:, 0] = u[:, 0]
    with np.errstate(all="ignore"):
        for k in range(K):
            z = np.concatenate([(cur - nav[:, k]) - x[:, k], ufly[:, k] - u[:, k]], axis=1)
            ufly[:, k + 1] = u[:, k + 1] + np.einsum("bji,bi->bj", np.asarray(gain, float)[:, k], z)
            S, _ = fr._substeps(dyn, par, cur, ufly[:, k], ufly[:, k + 1], sigma, dt, nsub)
            cur = S[:, -1]
            xfly[:, k + 1] = cur
    return xfly, ufly


def mc_check(xfly, ufly, eps, x, u, joint):
    """cov_reference.mc_check on the joint [z; eps]: (worst entry in standard errors, the same at node K, entries over 6) of the sample
    covariance of [xfly - x; ufly - u; eps] over N samples of ONE plan against joint [K+1][N][N]"""
    z = np.concatenate([xfly - x, ufly - u, eps], axis=-1)
    N = z.shape[0]
    z = z - z.mean(axis=0)
    Sh = np.einsum("bki,bkj->kij", z, z) / (N - 1)
    cov = np.asarray(joint, np.float64)
    dg = np.diagonal(cov, axis1=1, axis2=2)
    se = np.sqrt((dg[:, :, None] * dg[:, None, :] + cov ** 2) / (N - 1))
    diff = np.abs(Sh - cov)
    over = diff > 6.0 * se
    with np.errstate(all="ignore"):
        r = np.where(se > 0, diff / np.where(se > 0, se, 1.0), np.where(diff > 0, np.inf, 0.0))
    return float(r.max()), float(r[-1].max()), int(over.sum())
