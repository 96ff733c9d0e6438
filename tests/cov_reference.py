"""Independent CPU reference of the covariance analysis (scvx_cov_propagate_f64, include/scvx.h) -- a helper module, not a test file.

The recursion Sigma_{k+1} = M_k Sigma_k M_k' + diag(w, 0), M_k = F_k + G_k L_k, in numpy with the FULL augmented matrices F_k, G_k
(track_reference.fg) and the full M_k (the device kernel never forms M: it uses the block structure; this does not), with a `dtype`
argument: float64, or longdouble as the yardstick of the float64 rounding error.  The report columns come from closed-form
gradients of the six path functions; test_cov_cpu.py checks those gradients against central differences of flight_reference's own
path functions.  The gains are an argument: the tests feed track_reference.gains, never the device's.
"""
import numpy as np

import track_reference as tr

NREP = 16
COLUMNS = ("SIG_M", "SIG_R", "SIG_V", "SIG_Q", "SIG_W", "ELL_A", "ELL_B", "ELL_ANG", "SIG_PEAK", "S_THRUST", "N_MASS", "N_GLIDE", "N_TILT",
           "N_RATE", "N_TMAX", "N_TMIN")
IDX = {n: i for i, n in enumerate(COLUMNS)}
MARGINS = ("N_MASS", "N_GLIDE", "N_TILT", "N_RATE", "N_TMAX", "N_TMIN")
G_OF = {"N_MASS": "G_MASS", "N_GLIDE": "G_GLIDE", "N_TILT": "G_TILT", "N_RATE": "G_RATE", "N_TMAX": "G_TMAX", "N_TMIN": "G_TMIN"}


def s0_full(S0, B):
    """[B][14][14] from [B][14][14], one [14][14] or a [14] vector of standard deviations"""
    a = np.asarray(S0)
    if a.shape == (14,):
        a = np.diag(a * a)
    return np.broadcast_to(a, (B, 14, 14))


def propagate(deriv, K, gain, S0, w=None, dtype=np.float64):
    """cov [B][K+1][n][n] in `dtype`: every Sigma_k"""
    A, Bm, Bp = tr.split_tiles(deriv, K)
    B, nu = A.shape[0], Bm.shape[-1]
    n = 14 + nu
    S0 = s0_full(S0, B)
    W = np.zeros((n, n), dtype)
    if w is not None:
        W[np.arange(14), np.arange(14)] = np.broadcast_to(np.asarray(w), (14,)).astype(dtype)
    cov = np.zeros((B, K + 1, n, n), dtype)
    for b in range(B):
        S = np.zeros((n, n), dtype)
        s0 = S0[b].astype(dtype)
        S[:14, :14] = (s0 + s0.T) / 2
        cov[b, 0] = S
        for k in range(K):
            F, G = tr.fg(A[b, k].astype(dtype), Bm[b, k].astype(dtype), Bp[b, k].astype(dtype), dtype)
            M = F + G @ np.asarray(gain[b, k]).astype(dtype)
            T = M @ S @ M.T
            S = (T + T.T) / 2 + W
            cov[b, k + 1] = S
    return cov


def consts(p, dtype=np.float64):
    """(mdry, tggs, sqcm, omMax, Tmax, Tmin): the constants of the path functions as oracle/socp.py:99-101 forms them (float64 values,
    then cast: the device receives them as doubles)"""
    return tuple(dtype(v) for v in (p.mdry, np.tan(np.radians(p.gammaGs)), np.sqrt((1 - np.cos(np.radians(p.thetaMax))) / 2), p.omMax,
                                    p.Tmax, p.Tmin))


def path_g(p, xk, uk, dtype=np.float64):
    """the six path functions (g <= 0 satisfied) at one node, in the order of MARGINS"""
    mdry, tggs, sqcm, omMax, Tmax, Tmin = consts(p, dtype)
    xk, uk = np.asarray(xk, dtype), np.asarray(uk, dtype)
    nrm = lambda v: np.sqrt((v * v).sum())   # noqa: E731
    t = nrm(uk[:3])
    return np.array([mdry - xk[0], tggs * nrm(xk[2:4]) - xk[1], nrm(xk[9:11]) - sqcm, nrm(xk[11:14]) - omMax, t - Tmax, Tmin - t], dtype)


def path_grad(p, xk, uk, dtype=np.float64):
    """[6][n]: the gradients of path_g in z = [x; u], closed form; a row is NaN where the gradient is undefined (a norm exactly 0)"""
    mdry, tggs, sqcm, omMax, Tmax, Tmin = consts(p, dtype)
    xk, uk = np.asarray(xk, dtype), np.asarray(uk, dtype)
    n = 14 + uk.shape[0]
    c = np.zeros((6, n), dtype)
    nrm = lambda v: np.sqrt((v * v).sum())   # noqa: E731
    c[0, 0] = -1
    for row, sl, f in ((1, slice(2, 4), tggs), (2, slice(9, 11), 1), (3, slice(11, 14), 1)):
        r = nrm(xk[sl])
        c[row, sl] = f * xk[sl] / r if r != 0 else np.nan
    c[1, 1] = -1 if nrm(xk[2:4]) != 0 else np.nan
    t = nrm(uk[:3])
    e = uk[:3] / t if t != 0 else np.full(3, np.nan, dtype)
    c[4, 14:17] = e
    c[5, 14:17] = -e
    return c


def _sd(v):
    """square root of a variance: a rounded -1e-40 is 0, a NaN stays a NaN"""
    return np.sqrt(v) if v > 0 else (v if v != v else v * 0)


def report(p, x, u, cov, dtype=np.float64, detail=False):
    """[B][16] in `dtype` from the plan and every Sigma_k.  detail: also, per trajectory and margin, (node that attains the minimum,
    size of the terms of g there, s there) -- what the rounding floor of a margin is made of."""
    cov = np.asarray(cov, dtype)
    B, K1, n, _ = cov.shape
    x, u = np.asarray(x, dtype), np.asarray(u, dtype)
    cs = consts(p, dtype)
    out = np.zeros((B, NREP), dtype)
    det = [[None] * 6 for _ in range(B)]
    inf = dtype(np.inf)
    for b in range(B):
        SK = cov[b, -1]
        d = np.diag(SK)
        out[b, IDX["SIG_M"]] = _sd(d[0])
        out[b, IDX["SIG_R"]] = _sd(d[1:4].sum())
        out[b, IDX["SIG_V"]] = _sd(d[4:7].sum())
        out[b, IDX["SIG_Q"]] = _sd(d[7:11].sum())
        out[b, IDX["SIG_W"]] = _sd(d[11:14].sum())
        a, dd, h = SK[2, 2], SK[3, 3], SK[2, 3]
        mean, dif = (a + dd) / 2, (a - dd) / 2
        rad = np.sqrt(dif * dif + h * h)
        out[b, IDX["ELL_A"]] = _sd(mean + rad)
        out[b, IDX["ELL_B"]] = _sd(mean - rad)
        out[b, IDX["ELL_ANG"]] = np.arctan2(2 * h, a - dd) / 2
        out[b, IDX["SIG_PEAK"]] = max(_sd(np.trace(cov[b, k, :14, :14])) for k in range(K1))
        sT = dtype(0)
        N = [inf] * 6
        for k in range(1, K1):
            g = path_g(p, x[b, k], u[b, k], dtype)
            c = path_grad(p, x[b, k], u[b, k], dtype)
            t = np.sqrt((u[b, k, :3] ** 2).sum())
            terms = (max(abs(cs[0]), abs(x[b, k, 0])), max(abs(g[1] + x[b, k, 1]), abs(x[b, k, 1])), max(abs(g[2] + cs[2]), cs[2]),
                     max(abs(g[3] + cs[3]), cs[3]), max(t, cs[4]), max(t, cs[5]))
            for i in range(6):
                if np.isnan(c[i]).any():
                    continue
                s = _sd(c[i] @ cov[b, k] @ c[i])
                if i == 4:
                    sT = max(sT, s)
                if s == 0:
                    continue
                v = -g[i] / s
                if v < N[i] or v != v:
                    N[i] = v
                    det[b][i] = (k, float(terms[i]), float(s))
        out[b, IDX["S_THRUST"]] = sT
        for i, name in enumerate(MARGINS):
            out[b, IDX[name]] = N[i]
        if not np.isfinite(cov[b].astype(np.float64)).all():
            out[b] = np.nan
    return (out, det) if detail else out


def run(p, x, u, deriv, K, gain, S0, w=None, dtype=np.float64):
    """(report [B][16], cov [B][K+1][n][n], sig [B][K+1][n]) in `dtype`"""
    cov = propagate(deriv, K, gain, S0, w, dtype)
    d = np.diagonal(cov, axis1=-2, axis2=-1)
    sig = np.where(d > 0, np.sqrt(np.where(d > 0, d, 0)), np.where(d != d, d, 0))
    return report(p, x, u, cov, dtype), cov, sig


def open_loop_phi(deriv, K, dtype=np.float64):
    """Phi [B][14][14] = A_{K-1} ... A_0"""
    A, _, _ = tr.split_tiles(deriv, K)
    out = []
    for b in range(A.shape[0]):
        P = np.eye(14, dtype=dtype)
        for k in range(K):
            P = A[b, k].astype(dtype) @ P
        out.append(P)
    return np.stack(out)


def handover_s0(x0, seed=0, size=1e-3, scale=1.0):
    """The S0 = C C' of the checks: C = diag(sd)(I + 0.3 N), sd = size relative on r and v, size on q and w, the mass row zero, N standard
    normal from `seed`; `scale` multiplies the factor.  Returns (S0, C)."""
    sd = np.zeros(14)
    sd[1:7] = size * np.abs(np.asarray(x0, float)[1:7])
    sd[7:14] = size
    N = np.random.default_rng(seed).standard_normal((14, 14))
    C = scale * (np.diag(sd) @ (np.eye(14) + 0.3 * N))
    return C @ C.T, C


# ---- the two checks of the recursion against a flown closed loop (the C oracle on the CPU, scvx_track_fly_f64 on the device) ----
def rep(a, N):
    return np.repeat(a, N, axis=0)


def fd_covariance(fly, x, u, s, L, C, eps):
    """sum_j d_j d_j' at every node, d_j = (x+ - x-) / 2 eps for the starts x[0] +- eps C[:, j]; fly(x, u, s, L, dx0) -> xfly.
    One plan ([1][...] arrays) -> [K+1][14][14]"""
    dx0 = np.concatenate([eps * C.T, -eps * C.T])
    xf = fly(rep(x, 28), rep(u, 28), rep(s, 28), rep(L, 28), dx0)
    d = (xf[:14] - xf[14:]) / (2 * eps)
    return np.einsum("jki,jkl->kil", d, d)


def fd_errors(fly, x, u, s, L, cov, C, steps):
    """relative difference of the state block at node K between the finite-difference covariance and the recursion's, per step"""
    ref = cov[-1][:14, :14].astype(np.float64)
    return {e: float(np.abs(fd_covariance(fly, x, u, s, L, C, e)[-1] - ref).max() / np.abs(ref).max()) for e in steps}


def mc_check(xfly, ufly, x, u, cov):
    """(worst |S^ - Sigma| in standard errors over every entry of every node, the same at node K, number of entries over 6) of the
    sample covariance of [xfly - x; ufly - u] over N samples of ONE plan against cov [K+1][n][n]"""
    z = np.concatenate([xfly - x, ufly - u], axis=-1)   # [N][K+1][n]
    N = z.shape[0]
    z = z - z.mean(axis=0)
    Sh = np.einsum("bki,bkj->kij", z, z) / (N - 1)
    cov = cov.astype(np.float64)
    dg = np.diagonal(cov, axis1=1, axis2=2)
    se = np.sqrt((dg[:, :, None] * dg[:, None, :] + cov ** 2) / (N - 1))
    diff = np.abs(Sh - cov)
    over = diff > 6.0 * se
    with np.errstate(all="ignore"):
        r = np.where(se > 0, diff / np.where(se > 0, se, 1.0), np.where(diff > 0, np.inf, 0.0))
    return float(r.max()), float(r[-1].max()), int(over.sum())
