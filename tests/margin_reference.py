"""Independent CPU reference of the thrust-band back-offs (scvx_batch_set_thrust_margins, include/scvx.h) -- a helper module, not a
test file.

The conic subproblem of the independent oracle (oracle/socp.py: the rows of Rocketland.build_model, oracle/ipm.py: its own interior
point method) with the two edits of its right-hand side that the back-offs are:
    mtk_k <= Tmax - hi_k                                   rows h[K : 2K+1]          (rocketland.jl:186)
    -uhat_k' du_k <= -((Tmin + lo_k) - |ubar_k|)           rows h[3K+2 : 4K+3]       (rocketland.jl:199-201)
each asserted against the constant it overwrites; the SCvx loop is oracle.scvx.solve_step with oracle.scvx.solve_socp replaced for the
duration of the call; the per-node standard deviations of the path functions come from cov_reference.propagate and path_grad.
Nothing here reads the device.
"""
import contextlib

import numpy as np

import cov_reference as cr

PSIG_COLUMNS = ("MASS", "GLIDE", "TILT", "RATE", "THRUST")


def build(p, xbar, ubar, endpoint, deriv, rk, lo, hi):
    """oracle.socp.build with the back-offs lo, hi [K+1] applied to h"""
    from oracle import socp
    c, A, b, G, h, l, q, ix = socp.build(p, xbar, ubar, endpoint, deriv, rk)
    K = p.K
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    assert lo.shape == hi.shape == (K + 1,) and (lo >= 0).all() and (hi >= 0).all() and (lo + hi < p.Tmax - p.Tmin).all()
    un = np.array([np.linalg.norm(np.asarray(ubar)[k, :3]) for k in range(K + 1)])   # as socp.build forms it, row by row
    tmax_rows, tmin_rows = slice(K, 2 * K + 1), slice(K + 2 * (K + 1), K + 3 * (K + 1))
    assert np.array_equal(h[tmax_rows], np.full(K + 1, p.Tmax)), "the Tmax rows are not where they were"
    assert np.array_equal(h[tmin_rows], -(p.Tmin - un)), "the Tmin rows are not where they were"
    h = h.copy()
    h[tmax_rows] = p.Tmax - hi
    h[tmin_rows] = -((p.Tmin + lo) - un)
    return c, A, b, G, h, l, q, ix


def solve_socp(it, lo, hi, tol=1e-9):
    """oracle.scvx.solve_socp of the edited subproblem: (sol, ix)"""
    from oracle import ipm
    c, A, b, G, h, l, q, ix = build(it.problem, it.x, it.u, it.endpoint, it.deriv, it.rk, lo, hi)
    return ipm.solve(c, A, b, G, h, l, q, tol=tol), ix


@contextlib.contextmanager
def _patched(lo, hi):
    from oracle import scvx
    orig = scvx.solve_socp
    scvx.solve_socp = lambda it, tol=1e-9: solve_socp(it, lo, hi, tol)
    try:
        yield
    finally:
        scvx.solve_socp = orig


def solve_step(it, lo, hi, tol=1e-9):
    """oracle.scvx.solve_step with the edited subproblem"""
    from oracle import scvx
    with _patched(lo, hi):
        return scvx.solve_step(it, tol)


def solve(it, lo, hi, tol=1e-8):
    """Rocketland.solve_problem's loop (rocketland.jl:432-443) from the iterate `it` under the back-offs: (final iterate, cnu, cdel,
    log) with log one dict per step (accepted, cnu, cdel, rk, rho, ipm_iters)"""
    p = it.problem
    cnu = cdel = np.inf
    n, log = 1, []
    while (p.nuTol < cnu or p.delTol < cdel) and n < p.imax:
        prev = it
        it, cnu, cdel = solve_step(it, lo, hi, tol)
        log.append(dict(accepted=it.x is not prev.x, cnu=cnu, cdel=cdel, rk=it.rk, rho=it.last.get("rho"),
                        ipm_iters=it.last["sol"].iters))
        n += 1
    return it, cnu, cdel, log


def restart(p, x, u, sigma, ic=None, nsub=10):
    """the iterate of a re-plan: trajectory kept and re-linearised, rk = 100, cost = Inf, iter = 0 (create_initial's scalars)"""
    from dataclasses import replace
    from oracle import dynamics as od, scvx
    par = od.Params(p)
    e, d = od.linearize(par, x[None], u[None], np.array([float(sigma)]), 1.0 / (p.K + 1), nsub)
    if ic is not None:
        p = replace(p, rIi=np.asarray(ic[:3], float), vIi=np.asarray(ic[3:], float))
    return scvx.Iterate(p, par, float(sigma), np.array(x, float), np.array(u, float), e[0], d[0], 0, 100.0, np.inf, nsub)


def path_sigma(p, x, u, cov, dtype=np.float64):
    """psig [B][K+1][5] in `dtype`: s = sqrt(c' Sigma_k c) of the mass, glide-slope, tilt, rate and thrust-norm path functions at
    every node (gradients: cov_reference.path_grad, rows 0..4).  Node 0 is 0; a node whose gradient is undefined is 0; a trajectory
    with a non-finite Sigma anywhere is NaN."""
    cov = np.asarray(cov, dtype)
    B, K1 = cov.shape[:2]
    x, u = np.asarray(x, dtype), np.asarray(u, dtype)
    out = np.zeros((B, K1, 5), dtype)
    for b in range(B):
        for k in range(1, K1):
            c = cr.path_grad(p, x[b, k], u[b, k], dtype)
            for i in range(5):
                if not np.isnan(c[i]).any():
                    out[b, k, i] = cr._sd(c[i] @ cov[b, k] @ c[i])
        if not np.isfinite(cov[b].astype(np.float64)).all():
            out[b] = np.nan
    return out


def band_margins(p, u, lo, hi):
    """(smallest |u_k| - (Tmin + lo_k), smallest (Tmax - hi_k) - |u_k|) over the nodes: both >= 0 when the band holds"""
    t = np.linalg.norm(np.asarray(u)[..., :3], axis=-1)
    return float((t - (p.Tmin + lo)).min()), float(((p.Tmax - hi) - t).min())
