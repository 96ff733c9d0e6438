"""Independent CPU reference of the clamp-aware covariance analysis (scvx_cov_clamp_f64, include/scvx.h) -- a helper module, not a
test file.

The recursion of the header in numpy with the FULL augmented matrices F_k, G_k (track_reference.fg), the full N and the full
Mtilde_k = F_k + G_k N L_k (the device kernel never forms any of them), with a `dtype` argument: float64, or longdouble as the
yardstick of the float64 rounding error.  The float64 form takes erfc and exp from `math`; the longdouble form takes them from mpmath at
40 digits.  The gains are an argument: the tests feed track_reference.gains, never the device's.
"""
import math

import numpy as np

import cov_reference as cr
import track_reference as tr

NREP = 16
COLUMNS = ("SIG_M", "SIG_R", "SIG_V", "SIG_Q", "SIG_W", "BIAS_M", "BIAS_R", "BIAS_V", "BIAS_Q", "BIAS_W", "RMS_R", "RMS_V", "P_LO", "P_HI",
           "GAIN_MIN", "BIAS_PEAK")
IDX = {n: i for i, n in enumerate(COLUMNS)}
BLOCKS = {"M": slice(0, 1), "R": slice(1, 4), "V": slice(4, 7), "Q": slice(7, 11), "W": slice(11, 14)}


def _to_mp(v):
    """a longdouble as an mpmath number, exactly (two float64 pieces)"""
    import mpmath
    hi = float(v)
    if not math.isfinite(hi):
        return mpmath.mpf(hi)
    return mpmath.mpf(hi) + mpmath.mpf(float(np.longdouble(v) - np.longdouble(hi)))


def _from_mp(v):
    """an mpmath number as a longdouble, to the last bit of what two float64 pieces hold"""
    hi = float(v)
    if not math.isfinite(hi) or hi == 0.0:
        return np.longdouble(hi)
    return np.longdouble(hi) + np.longdouble(float(v - hi))


def _erfc_exp(dtype):
    """(erfc, exp) on scalars of `dtype`"""
    if dtype is np.longdouble:
        import mpmath

        def wrap(f):
            def g(v):
                with mpmath.workdps(40):
                    return _from_mp(f(_to_mp(v)))
            return g
        return wrap(mpmath.erfc), wrap(mpmath.exp)
    return (lambda v: dtype(math.erfc(float(v)))), (lambda v: dtype(math.exp(float(v))))


def sat_scalars(That, s, Tlo, Thi, dtype=np.float64, shift=False):
    """(P_lo, P_hi, gamma, E) of steps 4 and 5 for one node, with the special cases of the header: That == 0 (no clamp), s == 0 (the
    indicator forms), Thi = +inf (its term is 0 where P_hi == 0), Tlo == 0 (no lower clamp: P_lo = 0 and no phi(a)).  E = That + dE with
    dE = s (a P_lo + b P_hi + phi(a) - phi(b)), the header's form; shift: dE as a fifth value."""
    That, s, Tlo, Thi = dtype(That), dtype(s), dtype(Tlo), dtype(Thi)
    one, zero = dtype(1), dtype(0)
    ret = lambda plo, phi, gam, dE: (plo, phi, gam, That + dE) + ((dE,) if shift else ())   # noqa: E731
    if That == 0:
        return ret(zero, zero, one, zero)
    if s == 0:
        plo, phi = (one if That < Tlo else zero), (one if That > Thi else zero)
        return ret(plo, phi, (one if plo == 0 and phi == 0 else zero), min(max(That, Tlo), Thi) - That)
    erfc, exp = _erfc_exp(dtype)
    r2 = np.sqrt(dtype(2))
    i2p = 1 / np.sqrt(2 * (np.pi if dtype is not np.longdouble else _pi_ld()))
    with np.errstate(all="ignore"):
        a, b = (Tlo - That) / s, (Thi - That) / s
        plo, phi = (zero if Tlo == 0 else erfc(-a / r2) / 2), erfc(b / r2) / 2
        gam = 1 - plo - phi
        hi = zero if phi == 0 else b * phi
        pa = zero if Tlo == 0 else i2p * exp(-a * a / 2)
        dE = s * (a * plo + hi + (pa - i2p * exp(-b * b / 2)))
    return ret(plo, phi, gam, dE)


def _pi_ld():
    import mpmath
    with mpmath.workdps(40):
        return _from_mp(+mpmath.pi)


def _sd(v):
    return np.sqrt(v) if v > 0 else (v if v != v else v * 0)


def propagate(u, deriv, K, gain, S0, band, w=None, dtype=np.float64):
    """dict(cov [B][K+1][n][n], mean [B][K+1][n], satk [B][K][4] = (That, s, P_lo, P_hi) of node k + 1, gamma [B][K]) in `dtype`; u
    [B][K+1][nu] the plan's controls, band = (Tlo, Thi)"""
    A, Bm, Bp = tr.split_tiles(deriv, K)
    B, nu = A.shape[0], Bm.shape[-1]
    n = 14 + nu
    S0 = cr.s0_full(S0, B)
    Tlo, Thi = dtype(band[0]), dtype(band[1])
    W = np.zeros((n, n), dtype)
    if w is not None:
        W[np.arange(14), np.arange(14)] = np.broadcast_to(np.asarray(w), (14,)).astype(dtype)
    cov, mean = np.zeros((B, K + 1, n, n), dtype), np.zeros((B, K + 1, n), dtype)
    satk, gamma = np.zeros((B, K, 4), dtype), np.zeros((B, K), dtype)
    I3 = np.eye(3, dtype=dtype)
    with np.errstate(all="ignore"):
        for b in range(B):
            S = np.zeros((n, n), dtype)
            s0 = S0[b].astype(dtype)
            S[:14, :14] = (s0 + s0.T) / 2
            mu = np.zeros(n, dtype)
            cov[b, 0] = S
            for k in range(K):
                F, G = tr.fg(A[b, k].astype(dtype), Bm[b, k].astype(dtype), Bp[b, k].astype(dtype), dtype)
                L = np.asarray(gain[b, k]).astype(dtype)
                ub = np.asarray(u[b, k + 1]).astype(dtype)
                d = L @ mu
                chat = ub + d
                That = np.sqrt((chat[:3] * chat[:3]).sum())
                e = chat[:3] / That if That != 0 else np.zeros(3, dtype)
                g = L[:3].T @ e
                s = _sd(g @ S @ g)
                plo, phi, gam, E, dE = sat_scalars(That, s, Tlo, Thi, dtype, shift=True)
                if not (plo == 0 and phi == 0):
                    N = np.eye(nu, dtype=dtype)
                    N[:3, :3] = gam * np.outer(e, e) + (E / That) * (I3 - np.outer(e, e))
                    L = N @ L
                    d = d.copy()
                    d[:3] = d[:3] + dE * e   # E e - ubar = (That + dE) e - ubar = L mu + dE e
                mu = F @ mu + G @ d
                M = F + G @ L
                T = M @ S @ M.T
                S = (T + T.T) / 2 + W
                cov[b, k + 1], mean[b, k + 1] = S, mu
                satk[b, k], gamma[b, k] = (That, s, plo, phi), gam
    return {"cov": cov, "mean": mean, "satk": satk, "gamma": gamma}


def satrep(out, dtype=np.float64):
    """[B][16] in `dtype` from what propagate returns; a trajectory with a non-finite covariance is NaN throughout"""
    cov, mean, satk, gamma = (np.asarray(out[k], dtype) for k in ("cov", "mean", "satk", "gamma"))
    B, K = gamma.shape
    r = np.zeros((B, NREP), dtype)
    with np.errstate(all="ignore"):
        for b in range(B):
            dg, mu = np.diag(cov[b, -1]), mean[b, -1]
            for name, sl in BLOCKS.items():
                r[b, IDX["SIG_" + name]] = _sd(dg[sl].sum())
                r[b, IDX["BIAS_" + name]] = np.sqrt((mu[sl] * mu[sl]).sum())
            for name in ("R", "V"):
                sg, bs = r[b, IDX["SIG_" + name]], r[b, IDX["BIAS_" + name]]
                r[b, IDX["RMS_" + name]] = np.sqrt(sg * sg + bs * bs)
            r[b, IDX["P_LO"]], r[b, IDX["P_HI"]] = satk[b, :, 2].sum() / K, satk[b, :, 3].sum() / K
            r[b, IDX["GAIN_MIN"]] = np.nan if np.isnan(gamma[b]).any() else gamma[b].min()
            r[b, IDX["BIAS_PEAK"]] = np.sqrt((mean[b, :, :14] ** 2).sum(axis=1)).max()
            if not np.isfinite(cov[b].astype(np.float64)).all():
                r[b] = np.nan
    return r


def run(p, x, u, deriv, K, gain, S0, band=None, w=None, dtype=np.float64):
    """everything the device call returns, in `dtype`: dict(report [B][16] -- cov_reference.report on the clamp-aware Sigma_k --,
    satrep, mean, sig, covK, cov, satk, gamma); band None = the problem's (Tmin, Tmax)"""
    band = (p.Tmin, p.Tmax) if band is None else band
    out = propagate(u, deriv, K, gain, S0, band, w, dtype)
    d = np.diagonal(out["cov"], axis1=-2, axis2=-1)
    out["sig"] = np.where(d > 0, np.sqrt(np.where(d > 0, d, 0)), np.where(d != d, d, 0))
    out["covK"] = out["cov"][:, -1]
    out["report"] = cr.report(p, x, u, out["cov"], dtype)
    out["satrep"] = satrep(out, dtype)
    return out


# ---- the anchor: the recursion against sampled clamped flights ---------------------------------------------------------------------
def anchor_figures(SK_sl, muK_sl, plo_sl, phi_sl, SK_lin, xmean, xcov, out_lo, out_hi):
    """The figures of the four anchor conditions for ONE case: the statistically linearised landing covariance [14][14], mean [14] and
    mean shares P_LO, P_HI; the unclamped landing covariance; the sampled mean [14], covariance [14][14] of x_fly[K] - xbar[K] and the
    sampled shares OUT_LO, OUT_HI"""
    tr_ = lambda S, sl: float(np.trace(np.asarray(S, np.float64)[sl, sl]))   # noqa: E731
    mu, xm = np.asarray(muK_sl, np.float64), np.asarray(xmean, np.float64)
    return {"sl_r": tr_(SK_sl, BLOCKS["R"]) / tr_(xcov, BLOCKS["R"]), "sl_v": tr_(SK_sl, BLOCKS["V"]) / tr_(xcov, BLOCKS["V"]),
            "lin_r": tr_(SK_lin, BLOCKS["R"]) / tr_(xcov, BLOCKS["R"]), "lin_v": tr_(SK_lin, BLOCKS["V"]) / tr_(xcov, BLOCKS["V"]),
            "sl_m": float(SK_sl[0, 0] / xcov[0, 0]) if xcov[0, 0] > 0 else float("nan"),
            "sl_q": tr_(SK_sl, BLOCKS["Q"]) / tr_(xcov, BLOCKS["Q"]), "sl_w": tr_(SK_sl, BLOCKS["W"]) / tr_(xcov, BLOCKS["W"]),
            "bias_cos": float(mu @ xm / (np.linalg.norm(mu) * np.linalg.norm(xm))),
            "bias_ratio": float(np.linalg.norm(mu) / np.linalg.norm(xm)), "bias_sampled_r": float(np.linalg.norm(xm[1:4])),
            "p_lo": float(plo_sl / out_lo), "p_hi": float(phi_sl / out_hi)}


def anchor_assert(tag, f):
    """the four conditions, after printing every figure"""
    print("%s: " % tag + ", ".join("%s %.4g" % kv for kv in f.items()))
    assert 1.0 / 6.0 <= f["sl_r"] <= 6.0 and 1.0 / 6.0 <= f["sl_v"] <= 6.0, (tag, f["sl_r"], f["sl_v"])
    assert f["lin_v"] < 1.0 / 6.0, (tag, f["lin_v"])
    assert f["bias_cos"] >= 0.9, (tag, f["bias_cos"])
    assert 1.0 / 3.0 <= f["bias_ratio"] <= 3.0, (tag, f["bias_ratio"])
    assert 0.8 <= f["p_lo"] <= 2.0 and 0.8 <= f["p_hi"] <= 2.0, (tag, f["p_lo"], f["p_hi"])
