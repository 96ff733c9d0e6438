"""Independent CPU reference of plan tracking (scvx_track_gains_f64 / scvx_track_fly_f64, include/scvx.h) -- a helper module, not a
test file.

Gains: the backward Riccati recursion of the header, written with the full augmented matrices F_k = [[A, B-], [0, 0]] and
G_k = [B+; I] (the device kernel uses only the 14 x 14 block of P that meets the tile; this does not), in numpy with a `dtype`
argument: float64, or longdouble as the yardstick of the float64 rounding error.  numpy.linalg refuses longdouble, so the small
Cholesky solve is written by hand.

Closed loop: the feedback and the clamp are a few numpy lines at the nodes; the integrator between them is NOT restated: every
segment goes through flight_reference._substeps (the C oracle, or aero_torque_reference for the torque models), and the 16 columns
come from flight_reference.report.
"""
import numpy as np

import flight_reference as fr

CLAMP = 1
DEFAULT_WEIGHTS = (1.0, 1.0, 100.0)


def weights(nu, q=None, r=None, qf=None):
    d = DEFAULT_WEIGHTS
    return (np.broadcast_to(np.asarray(d[0] if q is None else q, float), (14,)).copy(),
            np.broadcast_to(np.asarray(d[1] if r is None else r, float), (nu,)).copy(),
            np.broadcast_to(np.asarray(d[2] if qf is None else qf, float), (14,)).copy())


def split_tiles(deriv, K):
    """deriv [B*K][14+2nu+1][14] (or [B][K][..]) -> A [B][K][14][14], Bm [B][K][14][nu], Bp [B][K][14][nu] (row = state component)"""
    d = np.asarray(deriv)
    ncol = d.shape[-2]
    nu = (ncol - 15) // 2
    d = d.reshape(-1, K, ncol, 14)
    t = np.swapaxes(d, -1, -2)   # [B][K][14][ncol]: element (i, j) of the column-major tile
    return t[..., :14], t[..., 14:14 + nu], t[..., 14 + nu:14 + 2 * nu]


def _chol_solve(S, H):
    """S [m][m] symmetric positive definite, H [m][c] -> S^-1 H, by hand in S's dtype"""
    m = S.shape[0]
    C = np.zeros_like(S)
    for j in range(m):
        for i in range(j, m):
            s = S[i, j] - C[i, :j] @ C[j, :j]
            C[i, j] = np.sqrt(s) if i == j else s / C[j, j]
    y = np.zeros_like(H)
    for i in range(m):
        y[i] = (H[i] - C[i, :i] @ y[:i]) / C[i, i]
    for i in range(m - 1, -1, -1):
        y[i] = (y[i] - C[i + 1:, i] @ y[i + 1:]) / C[i, i]
    return y


def fg(A, Bm, Bp, dtype=np.float64):
    """F [n][n], G [n][nu] of one segment"""
    nu = Bm.shape[-1]
    n = 14 + nu
    F = np.zeros((n, n), dtype)
    F[:14, :14] = A
    F[:14, 14:] = Bm
    G = np.zeros((n, nu), dtype)
    G[:14] = Bp
    G[14:] = np.eye(nu, dtype=dtype)
    return F, G


def gains(deriv, K, q=None, r=None, qf=None, dtype=np.float64):
    """(gain [B][K][nu][n], p0 [B][n][n]) in `dtype`"""
    A, Bm, Bp = split_tiles(deriv, K)
    B, nu = A.shape[0], Bm.shape[-1]
    n = 14 + nu
    q, r, qf = weights(nu, q, r, qf)
    Qz = np.zeros((n, n), dtype)
    Qz[np.arange(14), np.arange(14)] = q.astype(dtype)
    R = np.diag(r.astype(dtype))
    L = np.zeros((B, K, nu, n), dtype)
    P0 = np.zeros((B, n, n), dtype)
    for b in range(B):
        P = np.zeros((n, n), dtype)
        P[np.arange(14), np.arange(14)] = qf.astype(dtype)
        for k in range(K - 1, -1, -1):
            F, G = fg(A[b, k].astype(dtype), Bm[b, k].astype(dtype), Bp[b, k].astype(dtype), dtype)
            S = R + G.T @ P @ G
            H = G.T @ P @ F
            Lk = -_chol_solve(S, H)
            P = Qz + F.T @ P @ F + H.T @ Lk
            P = (P + P.T) / 2
            L[b, k] = Lk
        P0[b] = P
    return L, P0


def cost_identity(deriv, K, L, P0, q=None, r=None, qf=None, draws=4, seed=0):
    """Largest relative mismatch between z0' P0 z0 and the cost summed along z_{k+1} = (F_k + G_k L_k) z_k, over `draws` random z0 per
    trajectory; evaluated in longdouble so that only L and P0 carry error."""
    ld = np.longdouble
    A, Bm, Bp = split_tiles(deriv, K)
    B, nu = A.shape[0], Bm.shape[-1]
    n = 14 + nu
    q, r, qf = [w.astype(ld) for w in weights(nu, q, r, qf)]
    rng = np.random.default_rng(seed)
    worst = 0.0
    for b in range(B):
        for _ in range(draws):
            z0 = rng.uniform(-1.0, 1.0, n).astype(ld)
            z, J = z0.copy(), ld(0)
            for k in range(K):
                F, G = fg(A[b, k].astype(ld), Bm[b, k].astype(ld), Bp[b, k].astype(ld), ld)
                v = L[b, k].astype(ld) @ z
                J += (q * z[:14]) @ z[:14] + (r * v) @ v
                z = F @ z + G @ v
            J += (qf * z[:14]) @ z[:14]
            pred = z0 @ P0[b].astype(ld) @ z0
            worst = max(worst, float(abs(J - pred) / abs(J)) if J != 0 else float(abs(pred)))
    return worst


def clamp_control(p, un):
    """SCVX_TRACK_CLAMP on node controls un [B][nu] (in place): thrust norm into [Tmin, Tmax], fin norm below finmxf"""
    with np.errstate(all="ignore"):
        t = np.linalg.norm(un[:, :3], axis=1)
        f = np.where(t > p.Tmax, p.Tmax / t, np.where((t < p.Tmin) & (t > 0.0), p.Tmin / t, 1.0))
        un[:, :3] *= f[:, None]
        if un.shape[1] == 5:
            fn = np.linalg.norm(un[:, 3:5], axis=1)
            un[:, 3:5] *= np.where(fn > p.finmxf, p.finmxf / fn, 1.0)[:, None]
    return un


def chain(dyn, par, p, x, u, sigma, gain, dx0, nsub, flags=0):
    """closed loop: (samples [B][K][nsub+1][14], their controls [B][K][nsub+1][nu], xfly [B][K+1][14], ufly [B][K+1][nu],
    commanded thrust norms before the clamp [B][K])"""
    x, u, sigma = np.asarray(x, float), np.asarray(u, float), np.asarray(sigma, float)
    B, K1, _ = x.shape
    K = K1 - 1
    dt = 1.0 / (K + 1)
    nu = u.shape[-1]
    S, US = np.empty((B, K, nsub + 1, 14)), np.empty((B, K, nsub + 1, nu))
    ufly = np.empty((B, K1, nu))
    cmd = np.empty((B, K))
    cur = x[:, 0].copy() if dx0 is None else x[:, 0] + np.asarray(dx0, float)
    x0 = cur.copy()
    ufly[:, 0] = u[:, 0]
    with np.errstate(all="ignore"):
        for k in range(K):
            z = np.concatenate([cur - x[:, k], ufly[:, k] - u[:, k]], axis=1)
            un = u[:, k + 1] + np.einsum("bji,bi->bj", np.asarray(gain, float)[:, k], z)
            cmd[:, k] = np.linalg.norm(un[:, :3], axis=1)
            if flags & CLAMP:
                un = clamp_control(p, un)
            ufly[:, k + 1] = un
            S[:, k], US[:, k] = fr._substeps(dyn, par, cur, ufly[:, k], ufly[:, k + 1], sigma, dt, nsub)
            cur = S[:, k, -1]
    xfly = np.concatenate([x0[:, None], S[:, :, -1]], axis=1)
    return S, US, xfly, ufly, cmd


def fly(dyn, p, x, u, sigma, gain, dx0, nsub, flags=0, par=None):
    """(report [B][16], xfly, ufly, commanded thrust norms [B][K]) of the closed loop under problem p"""
    par = par if par is not None else dyn.Params(p)
    S, US, xfly, ufly, cmd = chain(dyn, par, p, x, u, sigma, gain, dx0, nsub, flags)
    return fr.report(p, x, S, US, xfly), xfly, ufly, cmd


def sensitivity(dyn, p, x, u, sigma, gain, dx0, nsub, eps, flags=0, draws=3, seed=0, par=None):
    """A_cl of the closed-loop chain, measured like flight_reference.sensitivity: re-run with the start perturbed by
    eps * xi, xi uniform in [-1, 1]^14 scaled by the start's own components; largest deviation of any node state / largest initial
    perturbation, worst trajectory and draw, floored at 1."""
    par = par if par is not None else dyn.Params(p)
    x = np.asarray(x, float)
    B = x.shape[0]
    d0 = np.zeros((B, 14)) if dx0 is None else np.asarray(dx0, float)
    rng = np.random.default_rng(seed)
    _, _, xf0, _, _ = chain(dyn, par, p, x, u, sigma, gain, d0, nsub, flags)
    A = 1.0
    for _ in range(draws):
        pert = (x[:, 0] + d0) * (eps * rng.uniform(-1.0, 1.0, (B, 14)))
        _, _, xf, _, _ = chain(dyn, par, p, x, u, sigma, gain, d0 + pert, nsub, flags)
        dev = np.abs(xf - xf0).max(axis=(1, 2))
        A = max(A, float((dev / np.abs(pert).max(axis=1)).max()))
    return A
