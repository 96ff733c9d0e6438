"""Independent CPU reference of the path-constraint back-offs (scvx_batch_set_path_margins, include/scvx.h) -- a helper module, not
a test file.

The conic subproblem of the independent oracle (oracle/socp.py: the rows of Rocketland.build_model, oracle/ipm.py: its own interior
point method) with the edits of its right-hand sides that the back-offs pm [K+1][4] = (mass, glide, tilt, rate) are.  The helper
equalities sit in b after the state, control, 25 boundary and 14 K dynamics rows, as K glide rows, K tilt rows and K rate rows:
    gshelp_k - r1_k / tan(gammaGs) = -glide_k           b[n0 + k]           k = 0..K-1    (rocketland.jl:142-144)
    aoa_help_k = sqcm - tilt_k                          b[n0 + K + k]                     (rocketland.jl:155-156)
    ang_sp_help_k = omMax - rate_k                      b[n0 + 2K + k]                    (rocketland.jl:163-164)
    -m_k <= -(mdry + mass_k)                            h[k - 1]            k = 1..K      (rocketland.jl:137)
each asserted against the constant it overwrites; the thrust edits are those of margin_reference.build.  The SCvx loop is
oracle.scvx.solve_step with oracle.scvx.solve_socp replaced for the duration of the call.  Nothing here reads the device.
"""
import contextlib

import numpy as np

import margin_reference as mr

MASS, GLIDE, TILT, RATE = range(4)
KINDS = ("mass", "glide", "tilt", "rate")


def consts(p):
    """(tan(gammaGs), sqcm) as oracle/socp.py:99-100 forms them"""
    return np.tan(np.radians(p.gammaGs)), np.sqrt((1 - np.cos(np.radians(p.thetaMax))) / 2)


def check_contract(p, pm):
    """the contract of the entries (include/scvx.h): raises AssertionError on a refusal"""
    K = p.K
    tggs, sqcm = consts(p)
    pm = np.asarray(pm, float)
    assert pm.shape == (K + 1, 4) and np.isfinite(pm).all() and (pm >= 0).all()
    assert (pm[:, TILT] < sqcm).all() and (pm[:, RATE] < p.omMax).all() and (pm[:, MASS] < p.mwet - p.mdry).all()
    assert not pm[K, [GLIDE, TILT, RATE]].any() and pm[0, MASS] == 0          # no such row
    assert pm[0, GLIDE] == 0 and pm[0, RATE] == 0                             # r and w are fixed at node 0
    return pm


def build(p, xbar, ubar, endpoint, deriv, rk, pm, lo=None, hi=None):
    """oracle.socp.build with the path back-offs pm [K+1][4] applied to b and h (and the thrust back-offs lo, hi [K+1] if given)"""
    K = p.K
    NU = 5 if getattr(p, "fins", False) else 3
    pm = check_contract(p, pm)
    z = np.zeros(K + 1)
    c, A, b, G, h, l, q, ix = mr.build(p, xbar, ubar, endpoint, deriv, rk, z if lo is None else lo, z if hi is None else hi)
    tggs, sqcm = consts(p)
    n0 = 14 * (K + 1) + NU * (K + 1) + 25 + 14 * K
    gl, ti, ra = slice(n0, n0 + K), slice(n0 + K, n0 + 2 * K), slice(n0 + 2 * K, n0 + 3 * K)
    assert b.shape[0] == n0 + 3 * K + (K + 1 if NU == 5 else 0)
    assert np.array_equal(b[gl], np.zeros(K)), "the glide-slope rows are not where they were"
    assert np.array_equal(b[ti], np.full(K, sqcm)), "the tilt rows are not where they were"
    assert np.array_equal(b[ra], np.full(K, p.omMax)), "the rate rows are not where they were"
    assert np.array_equal(h[:K], np.full(K, -p.mdry)), "the mass rows are not where they were"
    # the rows belong to the variables they are meant for: gshelp_k, aoa_help_k, ang_sp_help_k with coefficient 1, m_k with -1
    Ac, Gc = A.tocsr(), G.tocsr()
    for sl, var in ((gl, ix.gshelp), (ti, ix.aoa_help), (ra, ix.ang_sp_help)):
        assert all(Ac[sl.start + k, var[k]] == 1.0 for k in range(K))
    assert all(Gc[k - 1, ix.xv[0, k]] == -1.0 for k in range(1, K + 1))
    b, h = b.copy(), h.copy()
    b[gl] = -pm[:K, GLIDE]
    b[ti] = sqcm - pm[:K, TILT]
    b[ra] = p.omMax - pm[:K, RATE]
    h[:K] = -(p.mdry + pm[1:, MASS])
    return c, A, b, G, h, l, q, ix


def solve_socp(it, pm, lo=None, hi=None, tol=1e-9):
    """oracle.scvx.solve_socp of the edited subproblem: (sol, ix)"""
    from oracle import ipm
    c, A, b, G, h, l, q, ix = build(it.problem, it.x, it.u, it.endpoint, it.deriv, it.rk, pm, lo, hi)
    return ipm.solve(c, A, b, G, h, l, q, tol=tol), ix


@contextlib.contextmanager
def _patched(pm, lo, hi):
    from oracle import scvx
    orig = scvx.solve_socp
    scvx.solve_socp = lambda it, tol=1e-9: solve_socp(it, pm, lo, hi, tol)
    try:
        yield
    finally:
        scvx.solve_socp = orig


def solve_step(it, pm, lo=None, hi=None, tol=1e-9):
    """oracle.scvx.solve_step with the edited subproblem"""
    from oracle import scvx
    with _patched(pm, lo, hi):
        return scvx.solve_step(it, tol)


def solve(it, pm, lo=None, hi=None, tol=1e-8):
    """Rocketland.solve_problem's loop (rocketland.jl:432-443) from the iterate `it` under the back-offs: (final iterate, cnu, cdel,
    log) with log one dict per step (accepted, cnu, cdel, rk)"""
    p = it.problem
    cnu = cdel = np.inf
    n, log = 1, []
    while (p.nuTol < cnu or p.delTol < cdel) and n < p.imax:
        prev = it
        it, cnu, cdel = solve_step(it, pm, lo, hi, tol)
        log.append(dict(accepted=it.x is not prev.x, cnu=cnu, cdel=cdel, rk=it.rk))
        n += 1
    return it, cnu, cdel, log


def slacks(p, x, pm=None):
    """[K+1][4]: the slack of the four tightened rows at every node of the states x [K+1][14] (>= 0 when the row holds; +Inf where
    the node has no such row).  pm = None: the slacks of the true constraints."""
    K = p.K
    tggs, sqcm = consts(p)
    x = np.asarray(x, float)
    pm = np.zeros((K + 1, 4)) if pm is None else np.asarray(pm, float)
    s = np.full((K + 1, 4), np.inf)
    s[1:, MASS] = x[1:, 0] - (p.mdry + pm[1:, MASS])
    s[:K, GLIDE] = x[:K, 1] / tggs - pm[:K, GLIDE] - np.linalg.norm(x[:K, 2:4], axis=1)
    s[:K, TILT] = sqcm - pm[:K, TILT] - np.linalg.norm(x[:K, 9:11], axis=1)
    s[:K, RATE] = p.omMax - pm[:K, RATE] - np.linalg.norm(x[:K, 11:14], axis=1)
    return s


def margins_from_sigma(p, x, psig, nsigma, cap, kinds=KINDS):
    """pm [K+1][4] = min(nsigma s(k), cap width_k) of the kinds named, zeros elsewhere and where the contract demands them; the widths
    of scvx_batch_margins_from_cov: mwet - mdry, max(x_k[1], 0) / tan(gammaGs), sqcm, omMax.  psig [K+1][5] (MASS, GLIDE, TILT, RATE, .)"""
    K = p.K
    tggs, sqcm = consts(p)
    x, psig = np.asarray(x, float), np.asarray(psig, float)
    width = np.stack([np.full(K + 1, p.mwet - p.mdry), np.maximum(x[:, 1], 0.0) / tggs, np.full(K + 1, sqcm), np.full(K + 1, p.omMax)], axis=1)
    pm = np.zeros((K + 1, 4))
    for c, name in enumerate(KINDS):
        if name in kinds:
            pm[:, c] = np.minimum(nsigma * psig[:, c], cap * width[:, c])
    pm[K, [GLIDE, TILT, RATE]] = 0.0
    pm[0, [MASS, GLIDE, RATE]] = 0.0
    return pm
