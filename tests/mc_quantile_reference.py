"""Independent CPU reference of the order statistics and the per-node samples of the sampled dispersion (scvx_order_stats_f64,
scvx_track_mc_q_f64, include/scvx.h) -- a helper module, not a test file.

Per-node values: read off mc_reference.chain's outputs, nothing is flown here.  `xfly` [N][K+1][14] are the node states as node k's
feedback sees them (node 0 the start, node k >= 1 after the impulse of segment k - 1) and `cmd` [N][K] the commanded thrust norms before
the clamp, cmd[:, k - 1] the command FOR node k.  Quantiles: numpy's sort and a rank, never an interpolation."""
from statistics import NormalDist

import numpy as np

COLUMNS = ("MASS", "GLIDE", "TILT", "RATE", "THRUST")
IDX = {n: i for i, n in enumerate(COLUMNS)}
EPS = 2.0 ** -52


def tggs(p):
    return np.tan(np.deg2rad(p.gammaGs))


def path_values(p, xfly, cmd, u0):
    """[N][K+1][5]: the five path functions at every node of N flights -- MASS x[0], GLIDE tan(gammaGs) |r[2:3]| - r[1], TILT |q[3:4]|,
    RATE |w| (no constant subtracted), THRUST the commanded norm (node 0: |u0[0:3]|, the plan's own)"""
    xf, cmd = np.asarray(xfly, float), np.asarray(cmd, float)
    N, K1, _ = xf.shape
    v = np.empty((N, K1, 5))
    with np.errstate(all="ignore"):
        v[:, :, 0] = xf[:, :, 0]
        v[:, :, 1] = tggs(p) * np.sqrt(xf[:, :, 2] ** 2 + xf[:, :, 3] ** 2) - xf[:, :, 1]
        v[:, :, 2] = np.sqrt(xf[:, :, 9] ** 2 + xf[:, :, 10] ** 2)
        v[:, :, 3] = np.sqrt(xf[:, :, 11] ** 2 + xf[:, :, 12] ** 2 + xf[:, :, 13] ** 2)
        v[:, 0, 4] = np.linalg.norm(np.asarray(u0, float)[:3])
        v[:, 1:, 4] = cmd
    return v


def plan_values(p, x, u):
    """[K+1][5]: the same functions of the plan's own nodes x [K+1][14], u [K+1][nu]"""
    x, u = np.asarray(x, float), np.asarray(u, float)
    return path_values(p, x[None], np.linalg.norm(u[None, 1:, :3], axis=-1), u[0])[0]


def ranks(probs, S):
    """min(S - 1, max(0, ceil(p S) - 1)), written with integers where the product is exact: the reference of montecarlo.quantile_ranks"""
    return np.array([min(S - 1, max(0, int(np.ceil(float(q) * S)) - 1)) for q in np.atleast_1d(probs)], np.int64)


def order_stats(v, rk, axis=-1):
    """the elements of rank rk [nq] along `axis` in ascending order, NaNs last (numpy's sort); the rank axis comes last"""
    s = np.sort(np.moveaxis(np.asarray(v, float), axis, -1), axis=-1)
    return s[..., np.asarray(rk, np.int64)]


def quantile_se(prob, S):
    """standard error of the p-quantile of S normal draws in units of their standard deviation: sqrt(p (1 - p) / S) / phi(z_p)"""
    nd = NormalDist()
    return float(np.sqrt(prob * (1.0 - prob) / S) / nd.pdf(nd.inv_cdf(prob)))
