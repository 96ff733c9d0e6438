"""Independent CPU reference of the flight check (scvx_flight_check_f64, include/scvx.h) -- a helper module, not a test file.

It does not restate the integrator: it DRIVES one that exists.  `dyn` is a module with the interface of oracle.dynamics
(Params / propagate): oracle.dynamics itself (the C oracle) or, for the aerodynamic torque the oracle does not know,
tests/aero_torque_reference.py.  A segment of nsub RK4 substeps under a first-order hold is nsub one-substep segments of length
dt / nsub whose hold end points are the hold interpolated to the substep boundaries (interpolating a linear hold is exact, and the
mid-stage control of a substep is the mean of its two ends either way).  Chained over the whole trajectory this is single shooting
(SHOOT); restarted at every planned node it is the audit of the plan (PLAN).  The chain yields every sample state; the 16 numbers of
the report are then a few numpy lines with the constants of oracle/socp.py:99-101,188.

test_flight_cpu.py shows that the substep chain reproduces dyn.propagate(..., nsub) over whole segments to rounding.
"""
import numpy as np

SHOOT, PLAN = 0, 1
NREP = 16
COLUMNS = ("GAP", "MISS_R", "MISS_V", "MISS_Q", "MISS_W", "MASS_END", "G_MASS", "G_GLIDE", "G_TILT", "G_RATE", "G_TMAX", "G_TMIN",
           "G_GIMBAL", "G_DP", "G_FIN", "QNORM")
IDX = {n: i for i, n in enumerate(COLUMNS)}
STATE_COLUMNS = ("GAP", "MISS_R", "MISS_V", "MISS_Q", "MISS_W", "G_MASS", "G_GLIDE", "G_TILT", "G_RATE", "G_DP", "QNORM")


def _substeps(dyn, par, start, ua, ub, sigma, dt, nsub):
    """start [N][14], hold from ua to ub [N][nu] over a segment of length dt: the nsub + 1 states at the substep boundaries,
    [N][nsub+1][14], and the hold there, [N][nsub+1][nu]."""
    N = start.shape[0]
    lam = np.arange(nsub + 1) / nsub
    us = ua[:, None, :] * (1.0 - lam)[None, :, None] + ub[:, None, :] * lam[None, :, None]
    out = np.empty((N, nsub + 1, 14))
    out[:, 0] = start
    xx = np.zeros((N, 2, 14))
    for s in range(nsub):
        xx[:, 0] = out[:, s]
        out[:, s + 1] = dyn.propagate(par, xx, us[:, s:s + 2], sigma, dt / nsub, 1)[:, 0]
    return out, us


def chain(dyn, par, x, u, sigma, nsub, mode):
    """x [B][K+1][14], u [B][K+1][nu], sigma [B] -> (samples [B][K][nsub+1][14], their controls [B][K][nsub+1][nu],
    xfly [B][K+1][14]).  dt = 1 / (K + 1)."""
    x, u, sigma = np.asarray(x, float), np.asarray(u, float), np.asarray(sigma, float)
    B, K1, _ = x.shape
    K = K1 - 1
    dt = 1.0 / (K + 1)
    nu = u.shape[-1]
    with np.errstate(all="ignore"):
        if mode == PLAN:   # every segment starts at its planned node: all B * K segments at once
            S, US = _substeps(dyn, par, x[:, :-1].reshape(B * K, 14), u[:, :-1].reshape(B * K, nu), u[:, 1:].reshape(B * K, nu),
                              np.repeat(sigma, K), dt, nsub)
            S, US = S.reshape(B, K, nsub + 1, 14), US.reshape(B, K, nsub + 1, nu)
        else:
            S, US = np.empty((B, K, nsub + 1, 14)), np.empty((B, K, nsub + 1, nu))
            cur = x[:, 0].copy()
            for k in range(K):
                S[:, k], US[:, k] = _substeps(dyn, par, cur, u[:, k], u[:, k + 1], sigma, dt, nsub)
                cur = S[:, k, -1]
    xfly = np.concatenate([x[:, :1], S[:, :, -1]], axis=1)
    return S, US, xfly


def report(p, x, S, US, xfly):
    """The 16 columns from the sample states and controls; p: an oracle.model.DescentProblem (enforce_dp / fins select the
    optional rows)."""
    B = S.shape[0]
    tggs = np.tan(np.radians(p.gammaGs))                       # oracle/socp.py:99
    sqcm = np.sqrt((1 - np.cos(np.radians(p.thetaMax))) / 2)   # :100
    delMax = np.cos(np.radians(p.deltaMax))                    # :101
    n = np.linalg.norm
    s, c = S.reshape(B, -1, 14), US.reshape(B, -1, US.shape[-1])
    xe = xfly[:, -1]
    r = np.full((B, NREP), -np.inf)
    with np.errstate(all="ignore"):
        r[:, IDX["GAP"]] = np.abs(xfly[:, 1:] - np.asarray(x, float)[:, 1:]).max(axis=(1, 2))
        r[:, IDX["MISS_R"]] = n(xe[:, 1:4] - p.rIf, axis=-1)
        r[:, IDX["MISS_V"]] = n(xe[:, 4:7] - p.vIf, axis=-1)
        r[:, IDX["MISS_Q"]] = n(xe[:, 7:11] - p.qBIf, axis=-1)
        r[:, IDX["MISS_W"]] = n(xe[:, 11:14] - p.wBf, axis=-1)
        r[:, IDX["MASS_END"]] = xe[:, 0]
        r[:, IDX["G_MASS"]] = (p.mdry - s[..., 0]).max(axis=1)
        r[:, IDX["G_GLIDE"]] = (tggs * n(s[..., 2:4], axis=-1) - s[..., 1]).max(axis=1)
        r[:, IDX["G_TILT"]] = (n(s[..., 9:11], axis=-1) - sqcm).max(axis=1)
        r[:, IDX["G_RATE"]] = (n(s[..., 11:14], axis=-1) - p.omMax).max(axis=1)
        un = n(c[..., :3], axis=-1)
        r[:, IDX["G_TMAX"]] = (un - p.Tmax).max(axis=1)
        r[:, IDX["G_TMIN"]] = (p.Tmin - un).max(axis=1)
        r[:, IDX["G_GIMBAL"]] = (un - c[..., 0] / delMax).max(axis=1)
        if getattr(p, "enforce_dp", False):
            r[:, IDX["G_DP"]] = (n(s[..., 4:7], axis=-1) - float(np.sqrt(2.0 * p.dpMax / p.rho))).max(axis=1)   # :188
        if getattr(p, "fins", False):
            r[:, IDX["G_FIN"]] = (n(c[..., 3:5], axis=-1) - p.finmxf).max(axis=1)
        r[:, IDX["QNORM"]] = np.abs(n(s[..., 7:11], axis=-1) - 1.0).max(axis=1)
        # a non-finite sampled state (or node difference) makes the state columns NaN
        bad = ~np.isfinite(s).all(axis=(1, 2)) | ~np.isfinite(xfly[:, 1:] - np.asarray(x, float)[:, 1:]).all(axis=(1, 2))
    for name in STATE_COLUMNS:
        if name == "G_DP" and not getattr(p, "enforce_dp", False):
            continue
        r[bad, IDX[name]] = np.nan
    return r


def fly(dyn, p, x, u, sigma, nsub, mode, par=None):
    """(report [B][16], xfly [B][K+1][14]) of the plans (x, u, sigma) under problem p."""
    par = par if par is not None else dyn.Params(p)
    S, US, xfly = chain(dyn, par, x, u, sigma, nsub, mode)
    return report(p, x, S, US, xfly), xfly


def sensitivity(dyn, p, x, u, sigma, nsub, eps, draws=3, seed=0, par=None):
    """A of the SHOOT chain, measured from the reference alone: the chain re-run from x[0] (1 + eps xi), xi uniform in [-1, 1]^14,
    `draws` draws per trajectory; A = largest deviation at any node / largest initial perturbation, the worst trajectory and draw,
    floored at 1."""
    par = par if par is not None else dyn.Params(p)
    x, u, sigma = np.asarray(x, float), np.asarray(u, float), np.asarray(sigma, float)
    B = x.shape[0]
    rng = np.random.default_rng(seed)
    xi = rng.uniform(-1.0, 1.0, (draws, B, 14))
    xs = np.concatenate([x] + [x.copy() for _ in range(draws)])
    for d in range(draws):
        xs[(d + 1) * B:(d + 2) * B, 0] = x[:, 0] * (1.0 + eps * xi[d])
    _, _, xf = chain(dyn, par, xs, np.concatenate([u] * (draws + 1)), np.concatenate([sigma] * (draws + 1)), nsub, SHOOT)
    A = 1.0
    for d in range(draws):
        blk = slice((d + 1) * B, (d + 2) * B)
        dev = np.abs(xf[blk] - xf[:B]).max(axis=(1, 2))
        d0 = np.abs(xs[blk, 0] - x[:, 0]).max(axis=1)
        A = max(A, float((dev / d0).max()))
    return A


def g_lipschitz(p):
    """Factor by which an error of the state / control can grow in a G_* column: the 2-norm of up to 4 components (<= 2 x the
    largest) times the constant in front of it, plus the linear term."""
    return 2.0 * max(1.0, float(np.tan(np.radians(p.gammaGs)))) + max(1.0, 1.0 / float(np.cos(np.radians(p.deltaMax))))
