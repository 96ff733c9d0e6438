"""Independent CPU reference of the draws the device makes for the sampled dispersion (scvx_mc_draws_f64, scvx_track_mc_rng_f64,
include/scvx.h) -- a helper module, not a test file.

The words are numpy's own: np.random.Philox(key=seed, counter=[0, c1, c2, c3]).random_raw, one generator per (stream, plan, sample) --
nothing of montecarlo.philox4x64_blocks is used here.  The normals are the header's Box-Muller in np.longdouble (a 64-bit mantissa on
x86): u_j = ((w_j >> 11) + 0.5) 2^-53 formed in float64 as the device forms it (the sum rounds to even above 2^52; that rounding is part
of the draw's definition), then log, sqrt, and cos / sin of pi t after the EXACT reduction of the angle: 2 u is a multiple of 2^-52, so
its distance t to the nearest multiple of 1/2 is formed without rounding.  `dtype=np.float64` runs the same steps in float64."""
import numpy as np

STREAM_TRUTH, STREAM_NAV = 6, 7
PI_LD = np.longdouble("3.14159265358979323846264338327950288")


def words(seed, stream, c2, c3, nblocks):
    """blocks 0..nblocks-1 of the stream [0, stream, c2, c3] under key [seed, 0]: uint64 [nblocks][4]"""
    return np.random.Philox(key=int(seed), counter=[0, int(stream), int(c2), int(c3)]).random_raw(4 * nblocks).reshape(nblocks, 4)


def normals(w, dtype=np.longdouble):
    """[...][4] words -> [...][4] normals of `dtype`"""
    u = ((np.asarray(w, np.uint64) >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53          # float64, as the device
    out = np.empty(u.shape, dtype)
    pi = PI_LD if dtype is np.longdouble else dtype(np.pi)
    for a in (0, 2):
        r = np.sqrt(dtype(-2) * np.log(u[..., a].astype(dtype)))
        v = 2.0 * u[..., a + 1]                    # exact; in (0, 2]
        h = np.floor(2.0 * v + 0.5)                # the nearest multiple of 1/2 is h / 2 (ties upward: |t| = 1/4 either way)
        t = (v - 0.5 * h).astype(dtype)            # exact, in [-1/4, 1/4]
        ct, st = np.cos(pi * t), np.sin(pi * t)
        q = h.astype(np.int64) % 4
        out[..., a] = r * np.select([q == 0, q == 1, q == 2], [ct, -st, -ct], st)
        out[..., a + 1] = r * np.select([q == 0, q == 1, q == 2], [st, ct, -st], -ct)
    return out


def draws(seed, stream, samples, K, lo=0, plans=None, dtype=np.longdouble):
    """(start [P][S][14], nodes [P][S][K][14]) of `stream` for samples lo..lo+samples-1; plans None: shared draws (c2 = 0, P = 1), else
    the absolute plan indices (c2 = 1 + plan)"""
    c2s = [0] if plans is None else [1 + int(b) for b in plans]
    z = np.empty((len(c2s), samples, 1 + K, 16), dtype)
    for i, c2 in enumerate(c2s):
        for s in range(samples):
            z[i, s] = normals(words(seed, stream, c2, lo + s, 4 * (1 + K)), dtype).reshape(1 + K, 16)
    return z[:, :, 0, :14], z[:, :, 1:, :14]


def ulp_distance(a, ref):
    """|a - ref| in units of the float64 spacing at |ref|, entry by entry (a: float64, ref: longdouble)"""
    ref = np.asarray(ref, np.longdouble)
    sp = np.spacing(np.maximum(np.abs(ref).astype(np.float64), np.finfo(np.float64).tiny)).astype(np.longdouble)
    return (np.abs(np.asarray(a, np.float64).astype(np.longdouble) - ref) / sp).astype(np.float64)
