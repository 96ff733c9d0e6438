"""Independent CPU reference of the sampled closed-loop dispersion (scvx_track_mc_f64, include/scvx.h) -- a helper module, not a test
file.

Flights: track_reference.chain extended by the impulses of the header -- after segment k is integrated its end state receives
imp[:, k] (= sqrt(w) * eta) before node k + 1's gap, landing row and feedback see it; the s = nsub sample of segment k keeps the
undisturbed state.  The integrator is not restated: every segment goes through flight_reference._substeps (the C oracle, or
aero_torque_reference for the torque models), and the 16 columns come from flight_reference.report.

Reduction: the 48 columns of the report, the mean and the sample covariance of the landing deviation, in numpy from the dense
per-flight arrays.  The covariance is the two-pass form (deviations from the mean), not the device's two accumulated sums.
"""
import numpy as np

import flight_reference as fr
import track_reference as tr

NREP = 48
FLIGHT = fr.COLUMNS
COLUMNS = (tuple("MAX_" + n for n in FLIGHT) + tuple("MEAN_" + n for n in FLIGHT) + tuple("P_" + n[2:] for n in FLIGHT[6:15])
           + ("P_ANY", "OUT_LO", "OUT_HI", "N_BAD", "S"))
IDX = {n: i for i, n in enumerate(COLUMNS)}
EPS = 2.0 ** -52


def chain(dyn, par, p, x, u, sigma, gain, dx0, nsub, flags=0, imp=None):
    """track_reference.chain with impulses imp [N][K][14] or None: (samples [N][K][nsub+1][14] -- the last of a segment undisturbed --,
    their controls, xfly [N][K+1][14] -- the nodes, disturbed --, ufly [N][K+1][nu], commanded thrust norms before the clamp [N][K])"""
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
            z = np.concatenate([cur - x[:, k], ufly[:, k] - u[:, k]], axis=1)
            un = u[:, k + 1] + np.einsum("bji,bi->bj", np.asarray(gain, float)[:, k], z)
            cmd[:, k] = np.linalg.norm(un[:, :3], axis=1)
            if flags & tr.CLAMP:
                un = tr.clamp_control(p, un)
            ufly[:, k + 1] = un
            S[:, k], US[:, k] = fr._substeps(dyn, par, cur, ufly[:, k], ufly[:, k + 1], sigma, dt, nsub)
            cur = S[:, k, -1] if imp is None else S[:, k, -1] + imp[:, k]
            xfly[:, k + 1] = cur
    return S, US, xfly, ufly, cmd


def fly(dyn, p, x, u, sigma, gain, dx0, nsub, flags=0, imp=None, par=None):
    """(flights [N][16], xfly, ufly, commanded thrust norms [N][K]) of N flights, each with its own row of x, u, sigma, gain"""
    par = par if par is not None else dyn.Params(p)
    S, US, xfly, ufly, cmd = chain(dyn, par, p, x, u, sigma, gain, dx0, nsub, flags, imp)
    return fr.report(p, x, S, US, xfly), xfly, ufly, cmd


def fly_plan(dyn, p, xb, ub, sb, gb, dx0, nsub, flags=0, imp=None, par=None):
    """the same for N flights of ONE plan (xb [K+1][14], ub, sb a scalar, gb [K][nu][n]); the plan is broadcast, not copied"""
    N = np.shape(dx0)[0]
    bc = lambda a: np.broadcast_to(np.asarray(a, float), (N,) + np.shape(a))   # noqa: E731
    return fly(dyn, p, bc(xb), bc(ub), np.full(N, float(sb)), bc(gb), dx0, nsub, flags, imp, par)


def sensitivity(dyn, p, xb, ub, sb, gb, dx0, nsub, eps, flags=0, imp=None, draws=3, seed=0, par=None):
    """A_cl of the chain with impulses, measured like track_reference.sensitivity: starts perturbed by eps * xi scaled by the start's own
    components; largest deviation of any node state / largest initial perturbation, floored at 1"""
    par = par if par is not None else dyn.Params(p)
    d0 = np.asarray(dx0, float)
    rng = np.random.default_rng(seed)
    _, xf0, _, _ = fly_plan(dyn, p, xb, ub, sb, gb, d0, nsub, flags, imp, par)
    A = 1.0
    for _ in range(draws):
        pert = (np.asarray(xb, float)[0] + d0) * (eps * rng.uniform(-1.0, 1.0, d0.shape))
        _, xf, _, _ = fly_plan(dyn, p, xb, ub, sb, gb, d0 + pert, nsub, flags, imp, par)
        dev = np.abs(xf - xf0).max(axis=(1, 2))
        A = max(A, float((dev / np.abs(pert).max(axis=1)).max()))
    return A


def nan_max(a, axis=0):
    """the largest value, NaN if any is NaN (numpy's max already propagates; spelled out because the device's nan_max is the contract)"""
    a = np.asarray(a, float)
    return np.where(np.isnan(a).any(axis=axis), np.nan, np.max(np.where(np.isnan(a), -np.inf, a), axis=axis))


def out_counts(cmd, Tmin, Tmax, tol=0.0):
    """(low, high): numbers of commanded thrust norms cmd [...] with Tmin - t > tol and with t - Tmax > tol"""
    with np.errstate(invalid="ignore"):
        return int((Tmin - cmd > tol).sum()), int((cmd - Tmax > tol).sum())


def reduce(flights, e, n_lo, n_hi, K, tol=0.0):
    """(mcrep [48], xmean [14], xcov [14][14]) of ONE plan from its flights [S][16], landing deviations e [S][14] and the two counts of
    commanded node controls outside the band"""
    flights, e = np.asarray(flights, float), np.asarray(e, float)
    S = flights.shape[0]
    r = np.zeros(NREP)
    with np.errstate(all="ignore"):
        r[0:16] = nan_max(flights)
        r[16:32] = flights.sum(axis=0) / S
        over = flights[:, 6:15] > tol
        r[32:41] = over.sum(axis=0) / S
        r[41] = over.any(axis=1).sum() / S
        r[42], r[43] = n_lo / (S * K), n_hi / (S * K)
        r[44] = (~np.isfinite(flights[:, 0])).sum()
        r[45] = S
        xmean = e.sum(axis=0) / S
        d = e - xmean
        xcov = d.T @ d / (S - 1) if S > 1 else np.zeros((14, 14))
    return r, xmean, xcov


def se_check(xcov, cov, N):
    """(worst |xcov - cov| in standard errors over the 14 x 14 entries, number of entries over 6): cov_reference.mc_check's bound,
    Var(S^_ij) = (S_ii S_jj + S_ij^2) / (N - 1), on a landing covariance"""
    cov = np.asarray(cov, np.float64)
    dg = np.diag(cov)
    se = np.sqrt((dg[:, None] * dg[None, :] + cov ** 2) / (N - 1))
    diff = np.abs(np.asarray(xcov, np.float64) - cov)
    with np.errstate(all="ignore"):
        r = np.where(se > 0, diff / np.where(se > 0, se, 1.0), np.where(diff > 0, np.inf, 0.0))
    return float(r.max()), int((diff > 6.0 * se).sum())


def noise_for_equal_share(propagate, S0):
    """w [14] = alpha * diag(S0) with alpha such that the landing covariance from w alone has the trace of the one from S0 alone
    (both linear in their source); propagate(S0, w) -> Sigma_K [n][n].  Returns (w, trace from S0 alone, trace from w alone)."""
    d = np.diag(S0).copy()
    t0 = float(np.trace(propagate(S0, None)[:14, :14]))
    t1 = float(np.trace(propagate(np.zeros((14, 14)), d)[:14, :14]))
    w = d * (t0 / t1)
    return w, t0, float(np.trace(propagate(np.zeros((14, 14)), w)[:14, :14]))
