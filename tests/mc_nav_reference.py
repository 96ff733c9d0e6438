"""Independent CPU reference of the sampled closed-loop dispersion flown on a navigation estimate (scvx_track_mc_nav_f64,
include/scvx.h) -- a helper module, not a test file.

The error of the estimate: the linear recursion of the header in numpy, float64 or longdouble, from the same draws as the device
    eps_0 = CN xin,   eps+_k = eps_k - Kf_k (H eps_k + sqrt(rm) nud_k),   eps_{k+1} = A_k eps+_k (+ sqrt(w) eta_k)
Flights: mc_reference.chain with the law fed the estimate, z = [(cur - eps+_k) - xbar_k; u_k - ubar_k], and the impulses; the
integrator between the nodes is flight_reference._substeps (the C oracle), not restated.
Reduction: the mean and the covariance of [e; eps_K] in the two-pass form (deviations from the mean), not the device's two accumulated
sums, and the eight columns of the sampled navigation report read off that covariance.
"""
import numpy as np

import flight_reference as fr
import mc_reference as mr
import nav_reference as nr
import track_reference as tr

MCNAV_COLUMNS = ("NAV_M", "NAV_R", "NAV_V", "NAV_Q", "NAV_W", "MAX_FED", "EST_R", "EST_V")
MCNAV_IDX = {n: i for i, n in enumerate(MCNAV_COLUMNS)}


def eps_recursion(deriv_b, kf_b, H, rm, CN, xin, nud, w=None, eta=None, dtype=np.float64):
    """(fed [S][K][14] = eps+_k, before [S][K+1][14] = eps_k) of ONE plan in `dtype`: deriv_b [K][14+2nu+1][14] (column-major tiles), kf_b
    [K][14][m] or None, H [m][14] or None, rm [m], CN [14][14], xin [S][14], nud [S][K][m] or None, w [14] (variance) and eta
    [S][K][14] or None"""
    d = np.asarray(deriv_b).astype(dtype)
    K = d.shape[0]
    A = np.swapaxes(d[:, :14, :], 1, 2)                           # [k][row][column]
    m = 0 if H is None else int(np.shape(H)[0])
    xin = np.asarray(xin).astype(dtype)
    S = xin.shape[0]
    if m:
        Hm = np.asarray(H).astype(dtype).reshape(m, 14)
        sr = np.sqrt(np.broadcast_to(np.asarray(rm), (m,)).astype(dtype))
        kf = np.asarray(kf_b).astype(dtype).reshape(K, 14, m)
        nu_ = np.asarray(nud).astype(dtype)
    imp = None
    if w is not None and eta is not None:
        imp = np.asarray(eta).astype(dtype) * np.sqrt(np.broadcast_to(np.asarray(w), (14,)).astype(dtype))
    fed, before = np.zeros((S, K, 14), dtype), np.zeros((S, K + 1, 14), dtype)
    e = xin @ np.asarray(CN).astype(dtype).T
    with np.errstate(all="ignore"):
        for k in range(K):
            before[:, k] = e
            if m:
                e = e - (e @ Hm.T + sr * nu_[:, k]) @ kf[k].T
            fed[:, k] = e
            e = e @ A[k].T
            if imp is not None:
                e = e + imp[:, k]
        before[:, K] = e
    return fed, before


def chain(dyn, par, p, x, u, sigma, gain, dx0, nav, nsub, flags=0, imp=None):
    """mc_reference.chain with the law fed the estimate (nav [N][K][14] = eps+_k): the same five outputs"""
    x, u, sigma = np.asarray(x, float), np.asarray(u, float), np.asarray(sigma, float)
    B, K1, _ = x.shape
    K = K1 - 1
    dt = 1.0 / (K + 1)
    nu = u.shape[-1]
    S, US = np.empty((B, K, nsub + 1, 14)), np.empty((B, K, nsub + 1, nu))
    xfly, ufly = np.empty((B, K1, 14)), np.empty((B, K1, nu))
    cmd = np.empty((B, K))
    cur = x[:, 0].copy() if dx0 is None else x[:, 0] + np.asarray(dx0, float)
    xfly[:, 0] = cur
    ufly[:, 0] = u[:, 0]
    with np.errstate(all="ignore"):
        for k in range(K):
            z = np.concatenate([(cur - nav[:, k]) - x[:, k], ufly[:, k] - u[:, k]], axis=1)
            un = u[:, k + 1] + np.einsum("bji,bi->bj", np.asarray(gain, float)[:, k], z)
            cmd[:, k] = np.linalg.norm(un[:, :3], axis=1)
            if flags & tr.CLAMP:
                un = tr.clamp_control(p, un)
            ufly[:, k + 1] = un
            S[:, k], US[:, k] = fr._substeps(dyn, par, cur, ufly[:, k], ufly[:, k + 1], sigma, dt, nsub)
            cur = S[:, k, -1] if imp is None else S[:, k, -1] + imp[:, k]
            xfly[:, k + 1] = cur
    return S, US, xfly, ufly, cmd


def fly_plan(dyn, p, xb, ub, sb, gb, dx0, nav, nsub, flags=0, imp=None, par=None):
    """(flights [N][16], xfly, ufly, commanded thrust norms [N][K]) of N flights of ONE plan; the plan is broadcast, not copied"""
    par = par if par is not None else dyn.Params(p)
    N = np.shape(dx0)[0]
    bc = lambda a: np.broadcast_to(np.asarray(a, float), (N,) + np.shape(a))   # noqa: E731
    x = bc(xb)
    S, US, xfly, ufly, cmd = chain(dyn, par, p, x, bc(ub), np.full(N, float(sb)), bc(gb), dx0, nav, nsub, flags, imp)
    return fr.report(p, x, S, US, xfly), xfly, ufly, cmd


def sensitivity(dyn, p, xb, ub, sb, gb, dx0, nav, nsub, eps, flags=0, imp=None, draws=3, seed=0, par=None):
    """A_cl of the chain fed the estimate, measured like mc_reference.sensitivity: largest deviation of any node state / largest
    initial perturbation over `draws` perturbed starts, floored at 1"""
    par = par if par is not None else dyn.Params(p)
    d0 = np.asarray(dx0, float)
    rng = np.random.default_rng(seed)
    _, xf0, _, _ = fly_plan(dyn, p, xb, ub, sb, gb, d0, nav, nsub, flags, imp, par)
    A = 1.0
    for _ in range(draws):
        pert = (np.asarray(xb, float)[0] + d0) * (eps * rng.uniform(-1.0, 1.0, d0.shape))
        _, xf, _, _ = fly_plan(dyn, p, xb, ub, sb, gb, d0 + pert, nav, nsub, flags, imp, par)
        dev = np.abs(xf - xf0).max(axis=(1, 2))
        A = max(A, float((dev / np.abs(pert).max(axis=1)).max()))
    return A


def reduce(e, epsK, fed):
    """(jmean [28], jcov [28][28], mcnav [8]) of ONE plan from its landing deviations e [S][14], final errors epsK [S][14] and the fed
    errors fed [S][K][14]"""
    v = np.concatenate([np.asarray(e, float), np.asarray(epsK, float)], axis=1)
    S = v.shape[0]
    with np.errstate(all="ignore"):
        jmean = v.sum(axis=0) / S
        d = v - jmean
        jcov = d.T @ d / (S - 1) if S > 1 else np.zeros((28, 28))
        P, Cx = jcov[14:, 14:], jcov[:14, 14:]
        E = jcov[:14, :14] - Cx - Cx.T + P
        out = np.zeros(8)
        for name, key in (("NAV_M", "m"), ("NAV_R", "r"), ("NAV_V", "v"), ("NAV_Q", "q"), ("NAV_W", "w")):
            out[MCNAV_IDX[name]] = nr._sdv(np.diag(P)[nr.BLOCKS[key]].sum())
        out[MCNAV_IDX["MAX_FED"]] = mr.nan_max(np.abs(np.asarray(fed, float)).reshape(-1))
        out[MCNAV_IDX["EST_R"]] = nr._sdv(np.diag(E)[nr.BLOCKS["r"]].sum())
        out[MCNAV_IDX["EST_V"]] = nr._sdv(np.diag(E)[nr.BLOCKS["v"]].sum())
    return jmean, jcov, out


def joint_rows(n):
    """the rows and columns of the analysis's joint covariance Xi [N][N] (N = n + 14) that [e; eps_K] corresponds to: 0:14 and n:n+14"""
    return np.concatenate([np.arange(14), n + np.arange(14)])


def se_check(jcov, Xi, n, N):
    """mc_reference.se_check on the 28 x 28 joint: (worst entry in standard errors, entries over 6) of jcov against the rows and columns
    joint_rows(n) of Xi_K, for N samples"""
    ix = joint_rows(n)
    return mr.se_check(jcov, np.asarray(Xi, np.float64)[np.ix_(ix, ix)], N)
