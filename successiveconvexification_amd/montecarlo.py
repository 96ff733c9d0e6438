"""Monte-Carlo batches of independent initial-condition problems, sharded over the GPUs of a node.

New relative to the reference (which solves one trajectory serially): SURVEY.md 8d fixes the dispersion law, 8e the
sharding -- contiguous shards, one process per GPU, NO collective inside the SCvx iteration (solve_step reads no other
problem's data, rocketland.jl:226-321), one all-gather of the final trajectory records at the end.

The gather goes through the library's own RCCL communicator (scvx_comm_create / scvx_allgather_trajectories, what a
Julia host would call); `torch.distributed` is only the bootstrap channel for the 128-byte unique id and the clock
(barrier, max over ranks).  Everything here except the device calls runs unchanged on a CPU `gloo` group, which is how
tests/test_distributed_cpu.py drives it.
"""
import ctypes as C

import numpy as np


def disperse_ics(p, lo, hi, seed, frac=0.1):
    """rIi * (1 + frac U(-1,1)) and vIi * (1 + frac U(-1,1)) per component; trajectory b draws from Philox
    stream b of `seed`, so a shard [lo, hi) gets exactly the rows the whole batch would."""
    ic = np.zeros((hi - lo, 6))
    for b in range(lo, hi):
        rng = np.random.Generator(np.random.Philox(key=seed, counter=[0, 0, 0, b]))
        r = rng.uniform(-1.0, 1.0, size=6)
        ic[b - lo, 0:3] = np.asarray(p.rIi) * (1.0 + frac * r[0:3])
        ic[b - lo, 3:6] = np.asarray(p.vIi) * (1.0 + frac * r[3:6])
    return ic


def disperse_handover(x0, lo, hi, seed, frac_r=0.0, frac_v=0.0, angle=0.0, rate=0.0):
    """State offsets dx0 [hi - lo][14] at the handover to a tracking law (ScvxBatch.track, dynamics.track_fly_batch): where the
    vehicle really is when the plan starts at x0 ([hi - lo][14], or one [14] for all).  r and v relative per component
    (x0 * frac * U(-1,1)), the attitude a rotation by angle * U(-1,1) radians about a uniformly random axis, expressed as
    q (x) dq - q so that x0 + dx0 keeps a unit quaternion, rate * U(-1,1) added to each component of w, the mass untouched.
    Trajectory b draws from Philox stream b of `seed` (its own counter word, so the draws are not those of disperse_ics): a shard
    [lo, hi) gets exactly the rows the whole batch would."""
    x0 = np.broadcast_to(np.asarray(x0, np.float64), (hi - lo, 14))
    dx0 = np.zeros((hi - lo, 14))
    for b in range(lo, hi):
        rng = np.random.Generator(np.random.Philox(key=seed, counter=[1, 0, 0, b]))
        un = rng.uniform(-1.0, 1.0, size=10)
        ax = rng.standard_normal(3)
        ax /= np.linalg.norm(ax)
        i = b - lo
        dx0[i, 1:4] = x0[i, 1:4] * (frac_r * un[0:3])
        dx0[i, 4:7] = x0[i, 4:7] * (frac_v * un[3:6])
        th = angle * un[6]
        w, v = np.cos(0.5 * th), np.sin(0.5 * th) * ax
        qw, qv = x0[i, 7], x0[i, 8:11]
        dx0[i, 7] = (qw * w - qv @ v) - qw                      # Hamilton product q (x) dq, scalar first
        dx0[i, 8:11] = (qw * v + w * qv + np.cross(qv, v)) - qv
        dx0[i, 11:14] = rate * un[7:10]
    return dx0


def handover_factor(S0):
    """A factor C [14][14] with C C' = the symmetric part of S0: the Cholesky factor of the coordinates S0 disperses (a coordinate
    whose row of S0 is zero, e.g. an untouched mass, gets an exactly zero row, so its samples are exactly 0); where that block is
    only semi-definite, the eigen factor V sqrt(max(lambda, 0)) of the whole."""
    S = np.asarray(S0, np.float64)
    if S.shape == (14,):
        return np.diag(np.abs(S))
    if S.shape != (14, 14):
        raise ValueError("S0 must be [14][14] or a [14] vector of standard deviations")
    S = 0.5 * (S + S.T)
    live = np.flatnonzero(np.abs(S).max(axis=1) > 0.0)
    Cf = np.zeros((14, 14))
    if live.size == 0:
        return Cf
    try:
        Cf[np.ix_(live, live)] = np.linalg.cholesky(S[np.ix_(live, live)])
    except np.linalg.LinAlgError:
        lam, V = np.linalg.eigh(S)
        Cf = V * np.sqrt(np.maximum(lam, 0.0))[None, :]
    return Cf


def gaussian_handover(S0, lo, hi, seed):
    """Gaussian state offsets dx0 [hi - lo][14] with covariance S0 ([14][14], or a [14] vector of standard deviations) at the handover
    to a tracking law: the sampling counterpart of the covariance analysis (ScvxBatch.covariance, dynamics.cov_propagate_batch).
    dx0 = C xi with C = handover_factor(S0) and xi standard normal; trajectory b draws from Philox stream b of `seed` with a counter
    word of its own (the draws are neither those of disperse_ics nor of disperse_handover), so a shard [lo, hi) gets exactly the rows
    the whole batch would."""
    Cf = handover_factor(S0)
    dx0 = np.zeros((hi - lo, 14))
    for b in range(lo, hi):
        rng = np.random.Generator(np.random.Philox(key=seed, counter=[2, 0, 0, b]))
        dx0[b - lo] = Cf @ rng.standard_normal(14)
    return dx0


def mc_draws(samples, K, seed, noise=False, lo=0):
    """The draws of a sampled dispersion (dynamics.track_mc_batch, ScvxBatch.track_mc): (xi0 [samples][14], eta [samples][K][14] or
    None without `noise`), standard normal.  Sample s draws from Philox stream s of `seed` with a counter word of its own, 4 -- and in the
    SECOND counter word, which the generator's own increments of the first never reach, so the draws share nothing with those of
    disperse_ics, disperse_handover, gaussian_handover or nav_error_samples (words 0 to 3 in the first).  The 14 start draws come first, so
    xi0 does not depend on `noise`, and a shard [lo, lo + samples) gets exactly the rows the whole set would."""
    xi0 = np.empty((samples, 14))
    eta = np.empty((samples, K, 14)) if noise else None
    for s in range(samples):
        rng = np.random.Generator(np.random.Philox(key=seed, counter=[0, 4, 0, lo + s]))
        xi0[s] = rng.standard_normal(14)
        if noise:
            eta[s] = rng.standard_normal(K * 14).reshape(K, 14)
    return xi0, eta


def mc_nav_draws(samples, K, m, seed, lo=0):
    """The draws of the navigation error of a sampled dispersion flown on an estimate (dynamics.track_mc_nav_batch, ScvxBatch.track_mc
    with `nav`): (xin [samples][14] for eps_0, nud [samples][K][m] for the measurement noise, or None with m = 0), standard normal.
    Sample s draws from Philox stream s of `seed` with a counter word of its own, 5 in the SECOND word next to mc_draws' 4, so the draws
    share nothing with those of mc_draws (the same flight's start and process noise), nav_error_samples or the dispersion laws above.
    The 14 start draws come first, so xin does not depend on m, and a shard [lo, lo + samples) gets exactly the rows the whole set
    would."""
    xin = np.empty((samples, 14))
    nud = np.empty((samples, K, m)) if m else None
    for s in range(samples):
        rng = np.random.Generator(np.random.Philox(key=seed, counter=[0, 5, 0, lo + s]))
        xin[s] = rng.standard_normal(14)
        if m:
            nud[s] = rng.standard_normal(K * m).reshape(K, m)
    return xin, nud


_PHILOX_M0, _PHILOX_M1 = 0xD2E7470EE14C6C93, 0xCA5A826395121157
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B
MC_STREAM_TRUTH, MC_STREAM_NAV = 6, 7   # the second counter word of the device's two streams, beside mc_draws' 4 and mc_nav_draws' 5


def _mulhilo64(a, b):
    """(hi, lo) of the 128-bit product of the constant a (a Python int below 2^64) and the uint64 array b, by 32-bit halves"""
    m32, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    a0, a1 = np.uint64(a & 0xFFFFFFFF), np.uint64(a >> 32)
    b0, b1 = b & m32, b >> s32
    t = a0 * b0
    lo0, k = t & m32, t >> s32
    t = a1 * b0 + k
    w1, w2 = t & m32, t >> s32
    t = a0 * b1 + w1
    return a1 * b1 + w2 + (t >> s32), (t << s32) | lo0


def philox4x64_blocks(seed, c0, c1, c2, c3):
    """The Philox4x64-10 blocks of the counters [c0, c1, c2, c3] (uint64 arrays of one shape, or scalars that broadcast) under the key
    [seed, 0]: uint64 words [...][4], vectorised.  np.random.Philox(key=seed, counter=[0, c1, c2, c3]).random_raw(4 n) is the blocks of
    c0 = 1..n (numpy increments the counter before its first block); include/scvx.h spells out the round."""
    c0, c1, c2, c3 = (np.array(a, np.uint64) for a in np.broadcast_arrays(*(np.asarray(a, np.uint64) for a in (c0, c1, c2, c3))))
    k0, k1 = int(seed) & (2 ** 64 - 1), 0
    with np.errstate(over="ignore"):
        for _ in range(10):
            h0, l0 = _mulhilo64(_PHILOX_M0, c0)
            h1, l1 = _mulhilo64(_PHILOX_M1, c2)
            c0, c1, c2, c3 = h1 ^ c1 ^ np.uint64(k0), l1, h0 ^ c3 ^ np.uint64(k1), l0
            k0, k1 = (k0 + _PHILOX_W0) & (2 ** 64 - 1), (k1 + _PHILOX_W1) & (2 ** 64 - 1)
    return np.stack([c0, c1, c2, c3], axis=-1)


def box_muller(words, dtype=np.float64):
    """The normals of the device's draws from Philox words [...][4]: u_j = ((w_j >> 11) + 0.5) 2^-53 in float64 arithmetic (what the
    device forms; never 0), (z0, z1) = sqrt(-2 log u0) (cospi(2 u1), sinpi(2 u1)), (z2, z3) likewise from u2, u3 -> [...][4] of
    `dtype` (float64, or longdouble for the yardstick).  The angle is reduced EXACTLY before cos / sin: v = 2 u is dyadic, n = rint(2 v)
    and t = v - n / 2 in [-1/4, 1/4] without rounding, cos(pi v) and sin(pi v) from cos(pi t), sin(pi t) by the quarter turn n mod 4."""
    u = ((np.asarray(words, np.uint64) >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
    r = np.sqrt(-2 * np.log(u[..., 0::2].astype(dtype)))
    v = 2.0 * u[..., 1::2]
    n = np.rint(2.0 * v)
    t = (v - 0.5 * n).astype(dtype)
    pi = 4 * np.arctan(dtype(1))
    ct, st = np.cos(pi * t), np.sin(pi * t)
    q = n.astype(np.int64) & 3
    c = np.where(q == 0, ct, np.where(q == 1, -st, np.where(q == 2, -ct, st)))
    s = np.where(q == 0, st, np.where(q == 1, ct, np.where(q == 2, -st, -ct)))
    return np.stack([r * c, r * s], axis=-1).reshape(np.shape(words))


def _device_groups(seed, stream, samples, lo, plans, g0, g1, dtype=np.float64):
    """groups g0..g1-1 of `stream` for samples lo..lo+samples-1: [S][G][14] with shared draws (plans None), else [P][S][G][14] for the
    absolute plan indices `plans`"""
    if int(samples) < 1:
        raise ValueError("samples must be >= 1")
    c2 = np.zeros(1, np.uint64) if plans is None else np.uint64(1) + np.asarray(list(plans), np.uint64)
    c3 = np.uint64(int(lo) & (2 ** 64 - 1)) + np.arange(int(samples), dtype=np.uint64)
    j = np.uint64(1) + np.arange(4 * g0, 4 * g1, dtype=np.uint64)
    w = philox4x64_blocks(seed, j[None, None, :], np.uint64(stream), c2[:, None, None], c3[None, :, None])   # [P][S][4 G][4]
    z = box_muller(w, dtype).reshape(c2.size, int(samples), g1 - g0, 16)[..., :14]
    return z[0] if plans is None else z


def mc_draws_device(samples, K, seed, noise=False, lo=0, plans=None):
    """The float64 numpy twin of the draws the DEVICE makes with rng="device" (dynamics.track_mc_batch; the stream is spelled out in
    include/scvx.h): (xi0 [samples][14], eta [samples][K][14] or None without `noise`) with shared draws, [P][samples][..] for the
    absolute plan indices `plans` of independent draws.  lo: the first sample (sample_lo).  The words are numpy's Philox words
    (philox4x64_blocks against random_raw: tests/test_mc_rng_cpu.py), Box-Muller by box_muller; the device's log and sincospi differ from
    numpy's by a few ulp, so the device's own draws are dynamics.mc_draws_device_batch."""
    z = _device_groups(seed, MC_STREAM_TRUTH, samples, lo, plans, 0, 1 + (int(K) if noise else 0))
    return np.ascontiguousarray(z[..., 0, :]), (np.ascontiguousarray(z[..., 1:, :]) if noise else None)


def mc_nav_draws_device(samples, K, m, seed, lo=0, plans=None):
    """mc_draws_device for the navigation error: (xin [samples][14], nud [samples][K][m] or None with m = 0), the first m of the 14 draws
    of every node's group, so nud at m = 3 is the first three columns of nud at m = 14."""
    z = _device_groups(seed, MC_STREAM_NAV, samples, lo, plans, 0, 1 + (int(K) if m else 0))
    return np.ascontiguousarray(z[..., 0, :]), (np.ascontiguousarray(z[..., 1:, :int(m)]) if m else None)


def mc_vehicle_draws(samples, seed, lo=0):
    """The draws of the vehicle errors made on the HOST (vehicle= with rng="host"): zeta [samples][6], standard normal.  Sample s draws
    from Philox stream s of `seed` with 9 in the second counter word, beside mc_draws' 4 and mc_nav_draws' 5; a shard [lo, lo + samples)
    gets exactly the rows the whole set would."""
    zeta = np.empty((samples, 6))
    for s in range(samples):
        zeta[s] = np.random.Generator(np.random.Philox(key=seed, counter=[0, 9, 0, lo + s])).standard_normal(6)
    return zeta


MC_STREAM_VEH = 8   # the device's stream of the vehicle errors: the first six normals of its group 0


def mc_vehicle_draws_device(samples, seed, lo=0, plans=None):
    """mc_draws_device for the vehicle errors (dynamics.track_mc_batch(vehicle=, rng="device")): zeta [samples][6], or
    [P][samples][6] for the absolute plan indices `plans`, the first six normals of group 0 of stream 8; theta = mu + sp * zeta."""
    z = _device_groups(seed, MC_STREAM_VEH, samples, lo, plans, 0, 1)
    return np.ascontiguousarray(z[..., 0, :6])


VEHICLE_COMPONENTS = ("thrust", "mis_y", "mis_z", "isp", "aero", "fin")   # the SCVX_VEH_* order of include/scvx.h


def vehicle_errors(thrust=0.0, misalign=0.0, isp=0.0, aero=0.0, fin=0.0, mean=None):
    """(mu [6], sp [6]) of the per-flight vehicle errors theta = mu + sp * zeta (include/scvx.h "vehicle errors"), the vehicle= of the
    sampled calls: the 1 sigma of the relative thrust error, of the misalignment of the thrust axis (radians; a scalar for both body
    axes, or (about y, about z)), and of the relative errors of the specific impulse (alpha), of the aerodynamic scale (force_scalar)
    and of the fin forces.  mean: None (zero), or [6] in the same order.  aero needs an aerodynamic model, fin a model with fins: the
    library refuses a non-zero entry otherwise."""
    my, mz = (misalign, misalign) if np.ndim(misalign) == 0 else misalign
    sp = np.array([thrust, my, mz, isp, aero, fin], np.float64)
    mu = np.zeros(6) if mean is None else np.array(mean, np.float64)
    if mu.shape != (6,):
        raise ValueError("mean: [6] in the order " + ", ".join(VEHICLE_COMPONENTS))
    return mu, sp


def vehicle_budget(J, sp, covK):
    """Each component's share of the first-order landing variance Sigma_K + J diag(sp^2) J': J [14][6] = d x_K / d theta of the closed
    loop (dynamics.vehicle_sensitivity_batch), sp [6], covK [14][14] the landing covariance without vehicle errors (the [:14, :14] block
    of the analysis's).  Returns a dict: "cov" [14][14] the sum; "var" [7][14] the variance each of the six components and (row 6)
    covK contribute to each landing state, so var.sum(0) = diag(cov); "share" [7] the shares of the trace; "sigma_r" [7] and "sigma_v"
    [7] the root of each row's variance summed over position (states 1..3) and velocity (4..6).  First order: it ignores the O(theta^2)
    growth of the thrust norm under misalignment and every interaction."""
    J = np.asarray(J, np.float64)
    sp = np.asarray(sp, np.float64)
    cK = np.asarray(covK, np.float64)[:14, :14]
    if J.shape != (14, 6) or sp.shape != (6,) or cK.shape != (14, 14):
        raise ValueError("shape mismatch: J [14][6], sp [6], covK [14][14]")
    var = np.concatenate([(J * sp[None, :]).T ** 2, np.diag(cK)[None, :]])
    tot = var.sum()
    return {"cov": cK + (J * sp[None, :] ** 2) @ J.T, "var": var, "share": var.sum(1) / tot if tot > 0.0 else np.zeros(7),
            "sigma_r": np.sqrt(var[:, 1:4].sum(1)), "sigma_v": np.sqrt(var[:, 4:7].sum(1))}


def quantile_ranks(p, S):
    """The 0-based ascending ranks of the probabilities `p` (a scalar or an iterable) in a sample of S values, as the order statistics of
    the library count them (scvx_order_stats_f64, include/scvx.h): min(S - 1, max(0, ceil(p S) - 1)), numpy's method="inverted_cdf"
    with p = 0 the minimum and p = 1 the maximum.  A selection, never an interpolation.  Returns an int32 array [len(p)]."""
    pv = np.atleast_1d(np.asarray(p, np.float64))
    S = int(S)
    if S < 1:
        raise ValueError("quantile_ranks: S >= 1")
    if pv.ndim != 1 or not np.all((pv >= 0.0) & (pv <= 1.0)):
        raise ValueError("quantile_ranks: probabilities in [0, 1]")
    return np.clip(np.ceil(pv * S).astype(np.int64) - 1, 0, S - 1).astype(np.int32)


def quantile_stderr(p, S):
    """The standard error of the p-quantile estimated from S independent flights, in units of the quantity's standard deviation, under a
    NORMAL model: sqrt(p (1 - p) / S) / phi(z_p).  0.26 at p = 0.99865, S = 1,024: a tail quantile from S flights is itself uncertain."""
    from statistics import NormalDist
    nd = NormalDist()
    p = float(p)
    return float(np.sqrt(p * (1.0 - p) / int(S)) / nd.pdf(nd.inv_cdf(p)))


def path_functions(p, x, u):
    """The five path functions of psig / pathv (_lib.PSIG_COLUMNS) of the plan's own nodes: g [..][K+1][5] from x [..][K+1][14] and u
    [..][K+1][nu] -- MASS x[0], GLIDE tan(gammaGs) |r[2:3]| - r[1], TILT |q[3:4]|, RATE |w| (the constants of tilt and rate not
    subtracted) and THRUST |u[1:3]|.  p: the problem (gammaGs in degrees)."""
    x, u = np.asarray(x, np.float64), np.asarray(u, np.float64)
    tg = np.tan(np.deg2rad(p.gammaGs))
    return np.stack([x[..., 0], tg * np.sqrt(x[..., 2] ** 2 + x[..., 3] ** 2) - x[..., 1], np.sqrt(x[..., 9] ** 2 + x[..., 10] ** 2),
                     np.sqrt(x[..., 11] ** 2 + x[..., 12] ** 2 + x[..., 13] ** 2),
                     np.sqrt(u[..., 0] ** 2 + u[..., 1] ** 2 + u[..., 2] ** 2)], axis=-1)


def margins_from_quantiles(p, x, u, pathq_lo, pathq_hi, constraints="all", cap=0.25, current=None):
    """Per-node back-offs from the order statistics of a sampled closed loop (ScvxBatch.margins_from_mc): plain numpy.  p: the problem;
    x [B][K+1][14], u [B][K+1][nu]: the plans; pathq_lo / pathq_hi [B][K+1][5]: the Q_{1-p} and the Q_p order statistic of the five
    path functions at every node (one rank each of McReport.pathq).  With gbar_k = path_functions(p, x, u), the plan's own node:
        lo_k    = max(0, |ubar_k| - Q_{1-p}(T_k))        hi_k = max(0, Q_p(T_k) - |ubar_k|)        (the pair is ASYMMETRIC here)
        mass_k  = max(0, mbar_k - Q_{1-p}(m_k))          glide_k, tilt_k, rate_k = max(0, Q_p(g_k) - gbar_k)
    each capped by `cap` times the width scvx_batch_margins_from_cov uses: Tmax - Tmin, mwet - mdry, sqcm, omMax, and for the glide slope
    max(x_k[1], 0) / tan(gammaGs), which moves with the iterate.  Forced zeros as there: glide / tilt / rate at node K, mass / glide /
    rate at node 0.  A trajectory with a NaN quantile in a selected column gets zeros in every selected kind.  constraints: a subset of
    ("thrust", "mass", "glide", "tilt", "rate") or "all"; a kind that is not selected keeps the value of current = (lo, hi, pm) (zeros
    without it).  Returns (lo [B][K+1], hi [B][K+1], pm [B][K+1][4]).
    Limits: the glide back-off buys tan(gammaGs) times what is written, as the covariance one does; the quantiles carry the sampling
    error of quantile_stderr(p, S); the draws are shared across plans unless the call was made with independent=True; with the clamp on, T_k is still the UNCLAMPED command."""
    from ._lib import MARGIN_BITS, PMARG_INDEX, PMARG_N, PSIG_INDEX
    names = tuple(MARGIN_BITS) if isinstance(constraints, str) and constraints == "all" else tuple(constraints)
    if isinstance(constraints, str) and constraints != "all" or len(names) == 0 or any(n not in MARGIN_BITS for n in names):
        raise ValueError('constraints: a non-empty subset of %s, or "all"' % (tuple(MARGIN_BITS),))
    x, u = np.asarray(x, np.float64), np.asarray(u, np.float64)
    qlo, qhi = np.asarray(pathq_lo, np.float64), np.asarray(pathq_hi, np.float64)
    B, K1 = x.shape[0], x.shape[1]
    if x.shape != (B, K1, 14) or u.shape[:2] != (B, K1) or qlo.shape != (B, K1, 5) or qhi.shape != (B, K1, 5):
        raise ValueError("shape mismatch: x [B][K+1][14], u [B][K+1][nu], pathq_lo and pathq_hi [B][K+1][5]")
    if current is None:
        lo, hi, pm = np.zeros((B, K1)), np.zeros((B, K1)), np.zeros((B, K1, PMARG_N))
    else:
        lo, hi, pm = (np.array(a, np.float64) for a in current)
    g = path_functions(p, x, u)
    itan = 1.0 / np.tan(np.deg2rad(p.gammaGs))
    sqcm = np.sqrt((1.0 - np.cos(np.deg2rad(p.thetaMax))) / 2.0)
    iM, iG, iT, iR, iU = (PSIG_INDEX[n] for n in ("MASS", "GLIDE", "TILT", "RATE", "THRUST"))
    sel = [PSIG_INDEX[n.upper()] for n in names]
    bad = np.isnan(qlo[:, :, sel]).any(axis=(1, 2)) | np.isnan(qhi[:, :, sel]).any(axis=(1, 2))
    ok = ~bad[:, None]
    with np.errstate(invalid="ignore"):
        if "thrust" in names:
            w = cap * (p.Tmax - p.Tmin)
            lo[:] = np.where(ok, np.minimum(np.maximum(0.0, g[:, :, iU] - qlo[:, :, iU]), w), 0.0)
            hi[:] = np.where(ok, np.minimum(np.maximum(0.0, qhi[:, :, iU] - g[:, :, iU]), w), 0.0)
        if "mass" in names:
            v = np.where(ok, np.minimum(np.maximum(0.0, g[:, :, iM] - qlo[:, :, iM]), cap * (p.mwet - p.mdry)), 0.0)
            v[:, 0] = 0.0
            pm[:, :, PMARG_INDEX["MASS"]] = v
        if "glide" in names:
            width = np.maximum(x[:, :, 1], 0.0) * itan
            v = np.where(ok, np.minimum(np.maximum(0.0, qhi[:, :, iG] - g[:, :, iG]), cap * width), 0.0)
            v[:, 0] = v[:, K1 - 1] = 0.0
            pm[:, :, PMARG_INDEX["GLIDE"]] = v
        if "tilt" in names:
            v = np.where(ok, np.minimum(np.maximum(0.0, qhi[:, :, iT] - g[:, :, iT]), cap * sqcm), 0.0)
            v[:, K1 - 1] = 0.0
            pm[:, :, PMARG_INDEX["TILT"]] = v
        if "rate" in names:
            v = np.where(ok, np.minimum(np.maximum(0.0, qhi[:, :, iR] - g[:, :, iR]), cap * p.omMax), 0.0)
            v[:, 0] = v[:, K1 - 1] = 0.0
            pm[:, :, PMARG_INDEX["RATE"]] = v
    return lo, hi, pm


_STATE_BLOCKS = {"r": (1, 4), "v": (4, 7), "q": (7, 11), "w": (11, 14)}


def measurement_rows(names):
    """The measurement matrix H [m][14] of a navigation analysis (ScvxBatch.navigation, dynamics.nav_cov_batch) that observes whole
    state blocks directly: `names` is a string or an iterable out of "r", "v", "q", "w"; the rows are identity rows in state order."""
    names = list(names)
    if not set(names) <= set(_STATE_BLOCKS) or len(set(names)) != len(names):
        raise ValueError("measurement_rows: distinct names out of 'r', 'v', 'q', 'w', not %r" % (names,))
    rows = [i for nm in ("r", "v", "q", "w") if nm in names for i in range(*_STATE_BLOCKS[nm])]
    return np.eye(14)[rows]


def nav_error_samples(deriv_b, kf_b, H, rm, N0, lo, hi, seed):
    """Samples of the navigation error of ONE plan, the sampling counterpart of the navigation analysis: (fed [hi - lo][K][14], the
    error eps+_k of the updated estimate the law is fed at node k -- the `nav` of track_fly_batch / ScvxBatch.track --, and
    before [hi - lo][K+1][14], the error eps_k before the update), by the linear error recursion
        eps_0 = C xi (C = handover_factor(N0)),  eps+_k = J_k eps_k - Kf_k v_k  (J = I - Kf H, v ~ N(0, diag(rm))),  eps_{k+1} = A_k eps+_k
    with A_k the state block of the plan's tiles deriv_b [K][14+2nu+1][14] and kf_b [K][14][m] the filter gains of the analysis (H
    None or without rows: no update).  There is NO process noise: the flyer has none, so a sampled check against the analysis is a
    w = 0 check.  Sample b draws from Philox stream b of `seed` with a counter word of its own, so a shard [lo, hi) gets exactly the
    rows the whole batch would."""
    d = np.asarray(deriv_b, np.float64)
    K = d.shape[0]
    A = np.swapaxes(d[:, :14, :], 1, 2)                       # tiles are column-major: [k][column][row]
    m = 0 if H is None else int(np.shape(H)[0])
    Cf = handover_factor(N0)
    xi = np.empty((hi - lo, 14 + K * m))                      # per sample: 14 draws for eps_0, then m per node
    for b in range(lo, hi):
        xi[b - lo] = np.random.Generator(np.random.Philox(key=seed, counter=[3, 0, 0, b])).standard_normal(14 + K * m)
    if m:
        Hm = np.asarray(H, np.float64).reshape(m, 14)
        sr = np.sqrt(np.broadcast_to(np.asarray(rm, np.float64), (m,)))
        kf = np.asarray(kf_b, np.float64).reshape(K, 14, m)
    fed, before = np.zeros((hi - lo, K, 14)), np.zeros((hi - lo, K + 1, 14))
    e = xi[:, :14] @ Cf.T
    for k in range(K):
        before[:, k] = e
        if m:
            e = e - (e @ Hm.T + sr * xi[:, 14 + k * m:14 + (k + 1) * m]) @ kf[k].T
        fed[:, k] = e
        e = e @ A[k].T
    before[:, K] = e
    return fed, before


def shard_range(total: int, rank: int, world: int):
    """Contiguous shard [lo, hi) of `total` trajectories for `rank`; sizes differ by at most one."""
    base, rem = divmod(int(total), int(world))
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


class Shard:
    """This rank's part of a Monte-Carlo batch.  scaling = "weak": every rank holds `batch` trajectories (global =
    batch * world); "strong": `batch` is the GLOBAL count, split evenly (the all-gather needs equal shards)."""

    def __init__(self, problem, batch, seed, rank=0, world=1, scaling="weak"):
        if scaling not in ("weak", "strong"):
            raise ValueError("scaling must be 'weak' or 'strong'")
        if scaling == "strong" and batch % world:
            raise ValueError(f"strong scaling needs the global batch ({batch}) divisible by the world size ({world})")
        self.rank, self.world, self.scaling, self.seed = int(rank), int(world), scaling, int(seed)
        self.global_batch = batch * world if scaling == "weak" else batch
        self.lo, self.hi = shard_range(self.global_batch, rank, world)
        self.B = self.hi - self.lo
        self.ic = disperse_ics(problem, self.lo, self.hi, seed)


def bootstrap_comm(cache, dist, rank, world, lib=None):
    """scvx_comm_create on every rank: rank 0 draws the RCCL unique id, `dist` (any initialised torch.distributed
    group) broadcasts its 128 bytes.  Returns None on success, else the reason the native communicator is unavailable
    (the caller then falls back to a torch all-gather and says so)."""
    L = lib if lib is not None else cache._L
    # pre-flight, non-collective: ncclCommInitRank blocks until every rank has arrived, so a rank that cannot even bind
    # the library must be known to all of them BEFORE anyone enters it
    flags = [None] * world
    dist.all_gather_object(flags, int(L.scvx_comm_probe()))
    if any(f != 0 for f in flags):
        return "RCCL not loadable on rank(s) %s" % [i for i, f in enumerate(flags) if f != 0]
    buf = (C.c_char * 128)()
    ok = 1
    if rank == 0:
        ok = 1 if L.scvx_comm_unique_id(buf) == 0 else 0
    obj = [bytes(buf) if ok else None]
    dist.broadcast_object_list(obj, src=0)
    if obj[0] is None:
        return "scvx_comm_unique_id failed on rank 0 (RCCL not loadable)"
    rc = L.scvx_comm_create(cache.handle, C.c_char_p(obj[0]), int(rank), int(world))
    flags = [None] * world
    dist.all_gather_object(flags, int(rc))
    if any(f != 0 for f in flags):
        if rc == 0:
            L.scvx_comm_destroy(cache.handle)
        return "scvx_comm_create failed on rank(s) %s" % [i for i, f in enumerate(flags) if f != 0]
    return None


def gather_records(mine, dist=None, native=None):
    """All-gather of the per-rank records `mine` [B][n] (a torch tensor; equal B on every rank) into [world][B][n].
    native: callable(send_ptr, recv_ptr) -> rc enqueueing the library's RCCL all-gather on device tensors; without it
    the group's own backend is used (RCCL on GPU tensors, gloo on CPU tensors)."""
    import torch
    if dist is None or not dist.is_initialized():
        return mine.unsqueeze(0).clone()
    world = dist.get_world_size()
    out = torch.empty((world,) + tuple(mine.shape), dtype=mine.dtype, device=mine.device)
    if native is not None:
        rc = native(mine.data_ptr(), out.data_ptr())
        if rc != 0:
            raise RuntimeError(f"native all-gather failed ({rc})")
        return out
    if mine.is_cuda:
        dist.all_gather_into_tensor(out, mine.contiguous())
    else:
        parts = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(parts, mine.contiguous())
        out = torch.stack(parts)
    return out


def reduce_clock(elapsed, done, dist=None, device="cpu"):
    """(max over ranks of the timed interval, sum over ranks of the trajectory-iterations executed)."""
    import torch
    if dist is None or not dist.is_initialized():
        return float(elapsed), int(done)
    t = torch.tensor([elapsed], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    n = torch.tensor([float(done)], dtype=torch.float64, device=device)
    dist.all_reduce(n, op=dist.ReduceOp.SUM)
    return float(t.item()), int(n.item())


def flight_summary(report, status, tol=0.0):
    """What a Monte-Carlo batch has to say once it is solved and flown.  report: a dynamics.FlightReport or its raw [N][16] array
    (e.g. gathered over ranks with scvx_allgather_f64 and flattened); status [N]: the SCvx statuses of scvx_solve.  Returns a plain
    dict: counts by SCvx status, the number of converged plans, the share of them whose every G_* is <= tol, and min / median /
    p99 / max of GAP, MISS_R, MISS_V, MASS_END and each G_* over the converged plans (None where there is none).  Pure numpy."""
    from ._lib import FLIGHT_COLUMNS, FLIGHT_INDEX, FLIGHT_NREP
    names = {0: "converged", 1: "running", 2: "rejected", 3: "solver", 4: "nonfinite", 5: "infeasible"}
    raw = np.asarray(getattr(report, "raw", report), np.float64).reshape(-1, FLIGHT_NREP)
    status = np.asarray(status).reshape(-1)
    if status.shape[0] != raw.shape[0]:
        raise ValueError("report has %d rows, status %d" % (raw.shape[0], status.shape[0]))
    counts = {n: int(np.sum(status == c)) for c, n in names.items()}
    counts["other"] = int(status.shape[0] - sum(counts.values()))
    conv = raw[status == 0]
    gcols = [n for n in FLIGHT_COLUMNS if n.startswith("G_")]
    out = {"n": int(raw.shape[0]), "counts": counts, "converged": int(conv.shape[0]), "tol": float(tol), "stats": {}}
    if conv.shape[0]:
        g = conv[:, [FLIGHT_INDEX[n] for n in gcols]]
        ok = ~np.isnan(g).any(axis=1) & (np.nan_to_num(g, nan=np.inf).max(axis=1) <= tol)
        out["feasible_share"] = float(np.mean(ok))
    else:
        out["feasible_share"] = None
    for n in ["GAP", "MISS_R", "MISS_V", "MASS_END"] + gcols:
        c = conv[:, FLIGHT_INDEX[n]]
        if c.shape[0] == 0:
            out["stats"][n] = None
        elif np.all(np.isneginf(c)):   # a constraint the model does not enforce
            out["stats"][n] = {k: float("-inf") for k in ("min", "median", "p99", "max")}
        else:
            out["stats"][n] = {"min": float(np.min(c)), "median": float(np.median(c)), "p99": float(np.percentile(c, 99)),
                               "max": float(np.max(c))}
    return out


def audit_summary(rep, status, tol=1e-7):
    """What a Monte-Carlo batch has to say once its plans are audited segment by segment.  rep: a dynamics.SegmentReport or its seg
    [N][K][11] array; status [N]: the SCvx statuses of scvx_solve.  Returns a plain dict: the number of converged plans and, per G_*
    column over the converged plans, the share of plans and the share of segments with G > tol and the largest G (None where there is
    no converged plan; a NaN entry counts as a violation).  Pure numpy."""
    from ._lib import SEG_COLUMNS, SEG_INDEX, SEG_N
    seg = np.asarray(getattr(rep, "seg", rep), np.float64)
    if seg.ndim != 3 or seg.shape[2] != SEG_N:
        raise ValueError("seg must be [N][K][%d]" % SEG_N)
    status = np.asarray(status).reshape(-1)
    if status.shape[0] != seg.shape[0]:
        raise ValueError("seg has %d rows, status %d" % (seg.shape[0], status.shape[0]))
    conv = seg[status == 0]
    out = {"n": int(seg.shape[0]), "converged": int(conv.shape[0]), "tol": float(tol), "stats": {}}
    for n in (c for c in SEG_COLUMNS if c.startswith("G_")):
        g = conv[:, :, SEG_INDEX[n]]
        if g.shape[0] == 0:
            out["stats"][n] = None
            continue
        bad = ~(g <= tol)
        out["stats"][n] = {"plans": float(np.mean(bad.any(axis=1))), "segments": float(np.mean(bad)),
                           "max": float("nan") if np.isnan(g).any() else float(np.max(g))}
    return out


def dispersion_summary(covreport, status):
    """What a Monte-Carlo batch of plans has to say once its covariance analysis is done.  covreport: a dynamics.CovReport or its raw
    [N][16] array; status [N]: the SCvx statuses of scvx_solve.  Returns a plain dict: counts by SCvx status, the number of converged
    plans, and min / median / p99 / max of every column over the converged plans (None where there is none; a column that is +inf in
    every converged row -- no node had that margin -- reports +inf).  Pure numpy."""
    from ._lib import COV_COLUMNS, COV_INDEX, COV_NREP
    names = {0: "converged", 1: "running", 2: "rejected", 3: "solver", 4: "nonfinite", 5: "infeasible"}
    raw = np.asarray(getattr(covreport, "raw", covreport), np.float64).reshape(-1, COV_NREP)
    status = np.asarray(status).reshape(-1)
    if status.shape[0] != raw.shape[0]:
        raise ValueError("report has %d rows, status %d" % (raw.shape[0], status.shape[0]))
    counts = {n: int(np.sum(status == c)) for c, n in names.items()}
    counts["other"] = int(status.shape[0] - sum(counts.values()))
    conv = raw[status == 0]
    out = {"n": int(raw.shape[0]), "counts": counts, "converged": int(conv.shape[0]), "stats": {}}
    for n in COV_COLUMNS:
        c = conv[:, COV_INDEX[n]]
        if c.shape[0] == 0:
            out["stats"][n] = None
        elif np.all(np.isposinf(c)):
            out["stats"][n] = {k: float("inf") for k in ("min", "median", "p99", "max")}
        else:
            out["stats"][n] = {"min": float(np.min(c)), "median": float(np.median(c)), "p99": float(np.percentile(c, 99)),
                               "max": float(np.max(c))}
    return out


def clamp_summary(rep, status):
    """What a batch of plans has to say once its clamp-aware covariance analysis is done.  rep: a dynamics.SatCovReport or its satraw
    [N][16] array; status [N]: the SCvx statuses of scvx_solve.  Returns a plain dict: counts by SCvx status, the number of converged
    plans, and min / median / p99 / max of every column of _lib.SAT_COLUMNS over the converged plans (None where there is none).
    Pure numpy."""
    from ._lib import SAT_COLUMNS, SAT_INDEX, SAT_NREP
    names = {0: "converged", 1: "running", 2: "rejected", 3: "solver", 4: "nonfinite", 5: "infeasible"}
    raw = np.asarray(getattr(rep, "satraw", rep), np.float64).reshape(-1, SAT_NREP)
    status = np.asarray(status).reshape(-1)
    if status.shape[0] != raw.shape[0]:
        raise ValueError("report has %d rows, status %d" % (raw.shape[0], status.shape[0]))
    counts = {n: int(np.sum(status == c)) for c, n in names.items()}
    counts["other"] = int(status.shape[0] - sum(counts.values()))
    conv = raw[status == 0]
    out = {"n": int(raw.shape[0]), "counts": counts, "converged": int(conv.shape[0]), "stats": {}}
    for n in SAT_COLUMNS:
        c = conv[:, SAT_INDEX[n]]
        out["stats"][n] = None if c.shape[0] == 0 else {"min": float(np.min(c)), "median": float(np.median(c)),
                                                         "p99": float(np.percentile(c, 99)), "max": float(np.max(c))}
    return out


def mc_summary(rep, status):
    """What a batch of plans has to say once its sampled dispersion is done.  rep: a dynamics.McReport or its raw [N][48] array; status
    [N]: the SCvx statuses of scvx_solve.  Returns a plain dict: counts by SCvx status, the number of converged plans, the samples per
    plan, the number of converged plans with a non-finite flight, and min / median / p99 / max of every column over the converged plans
    (None where there is none; a column that is -inf in every converged row -- a constraint the model does not enforce -- reports
    -inf).  The statistics are over PLANS, each already reduced over its samples on the same draws.  Pure numpy."""
    from ._lib import MC_COLUMNS, MC_INDEX, MC_NREP
    names = {0: "converged", 1: "running", 2: "rejected", 3: "solver", 4: "nonfinite", 5: "infeasible"}
    raw = np.asarray(getattr(rep, "raw", rep), np.float64).reshape(-1, MC_NREP)
    status = np.asarray(status).reshape(-1)
    if status.shape[0] != raw.shape[0]:
        raise ValueError("report has %d rows, status %d" % (raw.shape[0], status.shape[0]))
    counts = {n: int(np.sum(status == c)) for c, n in names.items()}
    counts["other"] = int(status.shape[0] - sum(counts.values()))
    conv = raw[status == 0]
    out = {"n": int(raw.shape[0]), "counts": counts, "converged": int(conv.shape[0]),
           "samples": int(raw[0, MC_INDEX["S"]]) if raw.shape[0] else 0,
           "plans_with_bad_flights": int(np.sum(conv[:, MC_INDEX["N_BAD"]] != 0)), "stats": {}}
    for n in MC_COLUMNS:
        if n == "S":
            continue
        c = conv[:, MC_INDEX[n]]
        if c.shape[0] == 0:
            out["stats"][n] = None
        elif np.all(np.isneginf(c)):
            out["stats"][n] = {k: float("-inf") for k in ("min", "median", "p99", "max")}
        else:
            out["stats"][n] = {"min": float(np.min(c)), "median": float(np.median(c)), "p99": float(np.percentile(c, 99)),
                               "max": float(np.max(c))}
    return out
