"""Independent CPU reference of the vehicle errors in the first-order analyses (scvx_vehicle_tiles_f64, scvx_cov_vehicle_f64,
scvx_nav_cov_vehicle_f64, include/scvx.h) -- a helper module, not a test file.

  * Gamma_k's ISP and AERO columns (the vehicle tiles): central differences of the C oracle's one-segment flow from the planned node
    under the planned hold, the parameter sets scaled by mc_vehicle_reference.scaled_params, at steps h and h / 2, Richardson-
    extrapolated; the truncation estimate |value(h / 2) - extrapolate| comes back with them.  No variational equation is integrated.
  * The four tile identities (THRUST, MIS_Y, MIS_Z, FIN) straight from the oracle's tiles, and the same columns by central differences of
    the flow under the APPLIED control (mc_vehicle_reference.apply at the two ends of the hold).
  * J_0 = 0, J_{k+1} = M_k J_k + [Gamma_k; 0] with the FULL M_k = F_k + G_k L_k (track_reference.fg), and Sigma_k^tot = Sigma_k +
    J_k diag(sp^2) J_k' on top of cov_reference / nav_reference, float64 or longdouble.
"""
import numpy as np

import cov_reference as cr
import flight_reference as fr
import mc_vehicle_reference as vr
import nav_reference as nr
import track_reference as tr

H_FD = 2.0 ** -10


def rounding(K, h, A=1.0):
    """the project's rounding term of a central difference of step h through K segments of sensitivity A (mc_reference's K 1e-12 A_cl
    of a flown state, over the step)"""
    return K * 1e-12 * A / h


def _segments(x, u, s):
    B, K1, _ = x.shape
    K = K1 - 1
    nu = u.shape[-1]
    return x[:, :-1].reshape(-1, 14), u[:, :-1].reshape(-1, nu), u[:, 1:].reshape(-1, nu), np.repeat(np.asarray(s, float), K), 1.0 / (K + 1)


def _richardson(f, h):
    """central differences of f(t) at h and h / 2: (extrapolate, |value(h / 2) - extrapolate|)"""
    d = [(f(hh) - f(-hh)) / (2.0 * hh) for hh in (h, 0.5 * h)]
    ext = (4.0 * d[1] - d[0]) / 3.0
    return ext, np.abs(d[1] - ext)


def vtile_fd(dyn, p, par, x, u, s, nsub=10, h=H_FD):
    """(vtile [B][K][2][14], truncation estimate of the same shape): d x_{k+1} / d theta_ISP and / d theta_AERO (zeros without aerodynamics)"""
    X, U0, U1, S, dt = _segments(np.asarray(x, float), np.asarray(u, float), s)
    B, K = x.shape[0], x.shape[1] - 1
    out, trunc = np.zeros((B * K, 2, 14)), np.zeros((B * K, 2, 14))
    flow = lambda t3, t4: fr._substeps(dyn, vr.scaled_params(dyn, p, par, t3, t4), X, U0, U1, S, dt, nsub)[0][:, -1]   # noqa: E731
    out[:, 0], trunc[:, 0] = _richardson(lambda t: flow(t, 0.0), h)
    if getattr(p, "aero", None) is not None:
        out[:, 1], trunc[:, 1] = _richardson(lambda t: flow(0.0, t), h)
    return out.reshape(B, K, 2, 14), trunc.reshape(B, K, 2, 14)


def control_columns_fd(dyn, par, x, u, s, nsub=10, h=H_FD):
    """(Gamma [B][K][14][6] with the columns THRUST, MIS_Y, MIS_Z, FIN filled, truncation estimate): central differences of the flow
    under the applied control"""
    X, U0, U1, S, dt = _segments(np.asarray(x, float), np.asarray(u, float), s)
    B, K = x.shape[0], x.shape[1] - 1
    nu = u.shape[-1]
    out, trunc = np.zeros((B * K, 14, 6)), np.zeros((B * K, 14, 6))
    for c in (vr.THRUST, vr.MIS_Y, vr.MIS_Z) + ((vr.FIN,) if nu == 5 else ()):
        def flow(t, c=c):
            th = np.zeros((X.shape[0], 6))
            th[:, c] = t
            return fr._substeps(dyn, par, X, vr.apply(U0, th), vr.apply(U1, th), S, dt, nsub)[0][:, -1]
        out[:, :, c], trunc[:, :, c] = _richardson(flow, h)
    return out.reshape(B, K, 14, 6), trunc.reshape(B, K, 14, 6)


def gamma(deriv, u, vtile, dtype=np.float64):
    """Gamma [B][K][14][6] in `dtype`: the four tile identities of include/scvx.h and the two vehicle tiles"""
    u = np.asarray(u).astype(dtype)
    B, K1, nu = u.shape
    K = K1 - 1
    _, Bm, Bp = tr.split_tiles(deriv, K)
    Bm, Bp = Bm.astype(dtype), Bp.astype(dtype)
    G = np.zeros((B, K, 14, 6), dtype)
    ey, ez = np.array([0, 1, 0], dtype), np.array([0, 0, 1], dtype)
    for b in range(B):
        for k in range(K):
            u0, u1 = u[b, k], u[b, k + 1]
            G[b, k, :, vr.THRUST] = Bm[b, k][:, :3] @ u0[:3] + Bp[b, k][:, :3] @ u1[:3]
            G[b, k, :, vr.MIS_Y] = Bm[b, k][:, :3] @ np.cross(ey, u0[:3]) + Bp[b, k][:, :3] @ np.cross(ey, u1[:3])
            G[b, k, :, vr.MIS_Z] = Bm[b, k][:, :3] @ np.cross(ez, u0[:3]) + Bp[b, k][:, :3] @ np.cross(ez, u1[:3])
            if nu == 5:
                G[b, k, :, vr.FIN] = Bm[b, k][:, 3:5] @ u0[3:5] + Bp[b, k][:, 3:5] @ u1[3:5]
    if vtile is not None:
        vt = np.asarray(vtile).astype(dtype)
        G[:, :, :, vr.ISP] = vt[:, :, 0]
        G[:, :, :, vr.AERO] = vt[:, :, 1]
    return G


def sens(deriv, K, gain, Gam, dtype=np.float64):
    """J [B][K+1][n][6] in `dtype`: J_0 = 0, J_{k+1} = (F_k + G_k L_k) J_k + [Gamma_k; 0]"""
    A, Bm, Bp = tr.split_tiles(deriv, K)
    B, nu = A.shape[0], Bm.shape[-1]
    n = 14 + nu
    J = np.zeros((B, K + 1, n, 6), dtype)
    for b in range(B):
        for k in range(K):
            F, G = tr.fg(A[b, k].astype(dtype), Bm[b, k].astype(dtype), Bp[b, k].astype(dtype), dtype)
            M = F + G @ np.asarray(gain[b, k]).astype(dtype)
            J[b, k + 1] = M @ J[b, k]
            J[b, k + 1, :14] += np.asarray(Gam[b, k]).astype(dtype)
    return J


def rank6(J, sp, dtype=np.float64):
    """J_k diag(sp^2) J_k' [B][K+1][n][n]"""
    Js = np.asarray(J).astype(dtype) * np.asarray(sp).astype(dtype)[None, None, None, :]
    return np.einsum("bkic,bkjc->bkij", Js, Js)


def cov_run(p, x, u, deriv, K, gain, S0, sp, vtile, w=None, dtype=np.float64):
    """dict of the covariance form: cov0 (the plain Sigma_k), J, cov (Sigma_k^tot), sig, report, psig -- all in `dtype`"""
    import margin_reference as mg
    cov0 = cr.propagate(deriv, K, gain, S0, w, dtype)
    J = sens(deriv, K, gain, gamma(deriv, u, vtile, dtype), dtype)
    cov = cov0 + rank6(J, sp, dtype)
    d = np.diagonal(cov, axis1=-2, axis2=-1)
    sig = np.where(d > 0, np.sqrt(np.where(d > 0, d, 0)), 0)
    return dict(cov0=cov0, J=J, cov=cov, sig=sig, report=cr.report(p, x, u, cov, dtype), psig=mg.path_sigma(p, x, u, cov, dtype))


def nav_run(p, x, u, deriv, K, gain, S0, N0, H, rm, sp, vtile, w=None, dtype=np.float64):
    """dict of the navigation form: joint0 (the plain Xi_k), J, joint (J_k diag(sp^2) J_k' on the [z, z] block), report, navrep, psig"""
    import margin_reference as mg
    joint0, kf, _ = nr.propagate(deriv, K, gain, S0, N0, H, rm, w, dtype)
    n = joint0.shape[-1] - 14
    J = sens(deriv, K, gain, gamma(deriv, u, vtile, dtype), dtype)
    joint = joint0.copy()
    joint[:, :, :n, :n] += rank6(J, sp, dtype)
    zz = joint[:, :, :n, :n]
    return dict(joint0=joint0, J=J, joint=joint, kf=kf, report=cr.report(p, x, u, zz, dtype), navrep=nr.nav_report(joint, n, dtype),
                psig=mg.path_sigma(p, x, u, zz, dtype))


def sd_stderr(s, N):
    """standard error of a sample standard deviation of N normal samples about s"""
    return s / np.sqrt(2.0 * (N - 1))
