// Sampled closed-loop dispersion (scvx_track_mc_f64, include/scvx.h): S flights per plan under the tracking law of scvx_track.hip, with
// an optional impulse of process noise at every node, reduced on the device to one row of statistics per plan.  No counterpart in the
// reference.
//
// mc_fly_kernel: ONE LANE PER FLIGHT (plan b, sample s); the 64 lanes of a wavefront are 64 consecutive samples of the SAME plan, blocks
// of one wavefront, grid (ceil(S / 64), B).  Every read of the plan -- x, u, sigma, the gains -- is then one address for the whole
// wavefront (blockIdx.y and the loop counters only), which the compiler serves with scalar loads; only the draws xi0 / eta are per lane.
// scvx_track_fly_f64 spends its batch dimension on samples instead: every lane reads its own copy of the same 20 KB of gains.
//
// The flight arithmetic is fly_kernel<.., TRACK = true>'s (scvx_flight.hip), statement for statement: the feedback's fma order, the
// clamp, the first-order hold, the RK4 substep, the samples at s = 0..nsub, nan_max and the `bad` poison.  It is a kernel of its own and
// not one more template parameter there, so that the existing instantiations keep their code exactly (profiles/mc.md); without noise a
// flight's 16 columns are bitwise scvx_track_fly_f64's for the same plan and the same dx0 (tests/test_gpu_mc.py).
//
// Reduction, deterministic and without floating-point atomics: the wavefront reduces every statistic over its lanes with a fixed
// xor butterfly (32, 16, .., 1; lanes past S carry the neutral element) and lane 0 writes one partial row [MC_NP] per block into the
// context's workspace; mc_finish_kernel (one block per plan) combines the ceil(S / 64) partial rows of its plan in block order.  A lane
// past S flies sample S - 1 again, so that all 64 lanes reach the butterfly, and contributes nothing.
//
// PV (the last template parameter, as PS is for the covariance kernels): every live lane also stores the five path functions of psig at
// every node into pathv [B][K+1][5][S] -- the sample is the fastest index, so a wavefront's 64 samples store one contiguous line per
// value and each (b, k, f) row is contiguous for the order-statistics kernel (scvx_quantile.hip).  With PV off the instantiations keep
// the parent's registers, LDS and scratch (profiles/mc_quantiles.md) and are what the entry points without the _q launch.  The _q forms
// (scvx_track_mc_q_f64, include/scvx.h) follow the flight with order statistics of the flight columns and of the rows of pathv; flights
// and pathv live in a second workspace of the context when only their order statistics are asked for.
//
// RNG (the last template parameter): the loads of the draws xi0 and eta become calls of mc_draw_group (scvx_rng.hpp) -- every lane makes
// its own from Philox4x64-10, the four blocks of a group formed at the node and dead after it; everything else is statement for
// statement, so a flight is bitwise the flight of the RNG-off kernel fed the draws mc_draws_kernel dumps (tests/test_gpu_mc_rng.py).
// With RNG off the instantiations keep the parent's registers, LDS and scratch (profiles/mc_rng.md) and are what every entry point
// without _rng launches.
#include <cmath>
#include <limits>
#include "scvx_mc.hpp"   // the partial row, McK, the wavefront reductions and the draws made on the device, shared with scvx_mc_nav.hip

namespace scvx {

template <bool AERO, bool FIN, bool TRQ, bool PV, bool RNG>
__global__ __launch_bounds__(64) void mc_fly_kernel(DynPK<double, TRQ> p, PathK c, McK m, int S, int K, const double* __restrict__ x,
                                                    const double* __restrict__ u, const double* __restrict__ sigma,
                                                    const double* __restrict__ gain, const double* __restrict__ C0,
                                                    const double* __restrict__ xi0, const double* __restrict__ eta, double dt, int nsub,
                                                    int opt, double* __restrict__ part, double* __restrict__ flights,
                                                    double* __restrict__ xland, double* __restrict__ dx0o,
                                                    double* __restrict__ pathv, McRngK rg) {
    typedef double R;
    const int b = blockIdx.y;
    const int sl = blockIdx.x * 64 + threadIdx.x;
    const bool live = sl < S;
    const int s_ = live ? sl : S - 1;
    constexpr int NU = FIN ? 5 : 3;
    constexpr int n = 14 + NU;
    const R* xb = x + (size_t)b * (K + 1) * 14;
    const R* ub = u + (size_t)b * (K + 1) * NU;
    const R* gb = gain + (size_t)b * K * NU * n;
    const R* cb = C0 + (size_t)b * 196;
    const R* xi = RNG ? nullptr : xi0 + (size_t)s_ * 14;
    const R* et = (!RNG && eta) ? eta + (size_t)s_ * K * 14 : nullptr;
    const uint64_t rc2 = RNG ? mc_rng_c2(rg, b) : 0, rc3 = RNG ? mc_rng_c3(rg, s_) : 0;   // RNG: the flight's stream, scvx_rng.hpp
    const size_t fl = (size_t)b * S + s_;
    const R sig = sigma[b];
    const R h = dt / R(nsub);
    const R inv_n = R(1.0) / R(nsub);
    const R ninf = -std::numeric_limits<double>::infinity();
    const bool clamp = (opt & SCVX_TRACK_CLAMP) != 0;
    R xs[14], ukv[NU], upv[NU];
    // ---- the start: dx0 = C0 xi0, summed with fma in ascending j ----
    {
        R xv[16];
        if (RNG) {
            mc_draw_group(rg.seed, MC_STREAM_TRUTH, rc2, rc3, 0, 14, xv);
        } else {
#pragma unroll
            for (int j = 0; j < 14; j++) xv[j] = xi[j];
        }
#pragma unroll
        for (int i = 0; i < 14; i++) {
            R a = R(0.0);
#pragma unroll
            for (int j = 0; j < 14; j++) a = fma(cb[i * 14 + j], xv[j], a);
            if (dx0o && live) dx0o[fl * 14 + i] = a;
            xs[i] = a;
        }
    }
#pragma unroll
    for (int i = 0; i < 14; i++) xs[i] = xb[i] + xs[i];
#pragma unroll
    for (int j = 0; j < NU; j++) upv[j] = ub[j];
    R gap = R(0.0), bad = R(0.0);   // bad: 0 while every sampled state (and every node difference) is finite, else NaN
    R g_mass = ninf, g_glide = ninf, g_tilt = ninf, g_rate = ninf, g_tmax = ninf, g_tmin = ninf, g_gimbal = ninf, g_dp = ninf,
      g_fin = ninf, qn = R(0.0);
    int n_lo = 0, n_hi = 0;         // commanded node controls k = 1..K outside the thrust band by more than tol, before the clamp
    // PV: the five path functions at every node, pathv[((b (K + 1) + k) 5 + f) S + s] -- the sample is the fastest index, a wavefront
    // stores one contiguous line per value
    R* pvb = PV ? pathv + (size_t)b * (K + 1) * SCVX_PSIG_N * S + s_ : nullptr;
    if (PV && live) pvb[(size_t)SCVX_PSIG_THRUST * S] = sqrt(upv[0] * upv[0] + upv[1] * upv[1] + upv[2] * upv[2]);
    for (int k = 0; k < K; k++) {
        if (PV && live) mc_path_store(pvb + (size_t)k * SCVX_PSIG_N * S, S, c.tggs, xs);
        // ---- node k: the next node's control from the flown state and the applied control ----
        {
            R z[n];
#pragma unroll
            for (int i = 0; i < 14; i++) z[i] = xs[i] - xb[(size_t)k * 14 + i];
#pragma unroll
            for (int j = 0; j < NU; j++) {
                z[14 + j] = upv[j] - ub[(size_t)k * NU + j];
                ukv[j] = upv[j];
            }
            const R* g = gb + (size_t)k * NU * n;
#pragma unroll
            for (int j = 0; j < NU; j++) {
                R a = ub[(size_t)(k + 1) * NU + j];
#pragma unroll
                for (int i = 0; i < n; i++) a = fma(g[j * n + i], z[i], a);
                upv[j] = a;
            }
            {
                const R un = sqrt(upv[0] * upv[0] + upv[1] * upv[1] + upv[2] * upv[2]);
                n_lo += (c.Tmin - un > m.tol) ? 1 : 0;
                n_hi += (un - c.Tmax > m.tol) ? 1 : 0;
                if (PV && live) pvb[((size_t)(k + 1) * SCVX_PSIG_N + SCVX_PSIG_THRUST) * S] = un;
            }
            if (clamp) {
                const R un = sqrt(upv[0] * upv[0] + upv[1] * upv[1] + upv[2] * upv[2]);
                R f = R(1.0);
                if (un > c.Tmax) f = c.Tmax / un;
                else if (un < c.Tmin && un > R(0.0)) f = c.Tmin / un;
#pragma unroll
                for (int j = 0; j < 3; j++) upv[j] *= f;
                if (FIN) {
                    const R fn = sqrt(upv[3] * upv[3] + upv[4] * upv[4]);
                    const R ff = fn > c.finmxf ? c.finmxf / fn : R(1.0);
                    upv[3] *= ff;
                    upv[4] *= ff;
                }
            }
        }
        for (int s = 0; s <= nsub; s++) {
            // ---- sample: state xs, control of the hold at s / nsub (the stage-0 control of substep s) ----
            const R lk0 = R(s) * inv_n;
            R us[NU];
#pragma unroll
            for (int j = 0; j < NU; j++) us[j] = fma(ukv[j], R(1.0) - lk0, upv[j] * lk0);
            const R un = sqrt(us[0] * us[0] + us[1] * us[1] + us[2] * us[2]);
            g_tmax = nan_max(g_tmax, un - c.Tmax);
            g_tmin = nan_max(g_tmin, c.Tmin - un);
            g_gimbal = nan_max(g_gimbal, un - us[0] * c.inv_cosd);
            if (FIN) g_fin = nan_max(g_fin, sqrt(us[3] * us[3] + us[4] * us[4]) - c.finmxf);
            g_mass = nan_max(g_mass, c.mdry - xs[0]);
            g_glide = nan_max(g_glide, c.tggs * sqrt(xs[2] * xs[2] + xs[3] * xs[3]) - xs[1]);
            g_tilt = nan_max(g_tilt, sqrt(xs[9] * xs[9] + xs[10] * xs[10]) - c.sqcm);
            g_rate = nan_max(g_rate, sqrt(xs[11] * xs[11] + xs[12] * xs[12] + xs[13] * xs[13]) - c.omMax);
            if (c.dp) g_dp = nan_max(g_dp, sqrt(xs[4] * xs[4] + xs[5] * xs[5] + xs[6] * xs[6]) - c.vmax);
            qn = nan_max(qn, fabs(sqrt(xs[7] * xs[7] + xs[8] * xs[8] + xs[9] * xs[9] + xs[10] * xs[10]) - R(1.0)));
#pragma unroll
            for (int i = 0; i < 14; i++) bad = fma(xs[i], R(0.0), bad);
            if (s == nsub) break;
            // ---- one RK4 substep, as propagate_kernel takes it ----
            R xa[14], xt[14];
#pragma unroll
            for (int i = 0; i < 14; i++) {
                xa[i] = xs[i];
                xt[i] = xs[i];
            }
#pragma unroll
            for (int stg = 0; stg < 4; stg++) {
                const R lkp = (R(s) + (stg == 0 ? R(0.0) : (stg == 3 ? R(1.0) : R(0.5)))) * inv_n;
                const R lkm = R(1.0) - lkp;
                R uu[NU];
#pragma unroll
                for (int j = 0; j < NU; j++) uu[j] = fma(ukv[j], lkm, upv[j] * lkp);
                R g[14];
                rhs_only<AERO, FIN, TRQ>(p, xt, uu, g);
                const R wacc = h * ((stg == 0 || stg == 3) ? (R(1.0) / R(6.0)) : (R(1.0) / R(3.0)));
                const R wnext = h * (stg == 2 ? R(1.0) : R(0.5));
#pragma unroll
                for (int i = 0; i < 14; i++) {
                    const R dx = sig * g[i];
                    xa[i] = fma(wacc, dx, xa[i]);
                    if (stg < 3) xt[i] = fma(wnext, dx, xs[i]);
                }
            }
#pragma unroll
            for (int i = 0; i < 14; i++) xs[i] = xa[i];
        }
        // ---- the impulse of segment k: after its last sample, before node k + 1's gap, dense row and feedback ----
        if (RNG) {
            if (rg.noise) {
                R ev[16];   // group 1 + k, formed here and dead after the impulse
                mc_draw_group(rg.seed, MC_STREAM_TRUTH, rc2, rc3, 1 + k, 14, ev);
#pragma unroll
                for (int i = 0; i < 14; i++) xs[i] = fma(m.sw[i], ev[i], xs[i]);
            }
        } else if (et) {
#pragma unroll
            for (int i = 0; i < 14; i++) xs[i] = fma(m.sw[i], et[(size_t)k * 14 + i], xs[i]);
        }
        // ---- node k + 1: the flown state against the planned one ----
        const R* xn = xb + (size_t)(k + 1) * 14;
#pragma unroll
        for (int i = 0; i < 14; i++) {
            const R d = xs[i] - xn[i];
            gap = nan_max(gap, fabs(d));
            bad = fma(d, R(0.0), bad);
        }
    }
    // xs is the flown final node
    if (PV && live) mc_path_store(pvb + (size_t)K * SCVX_PSIG_N * S, S, c.tggs, xs);
    R mr = R(0.0), mv = R(0.0), mq = R(0.0), mw = R(0.0);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const R dr = xs[1 + i] - c.rIf[i], dv = xs[4 + i] - c.vIf[i], dw = xs[11 + i] - c.wBf[i];
        mr = fma(dr, dr, mr); mv = fma(dv, dv, mv); mw = fma(dw, dw, mw);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) { const R dq = xs[7 + i] - c.qBIf[i]; mq = fma(dq, dq, mq); }
    R o[SCVX_FLIGHT_NREP];
    o[SCVX_FLIGHT_GAP] = gap + bad;
    o[SCVX_FLIGHT_MISS_R] = sqrt(mr) + bad;
    o[SCVX_FLIGHT_MISS_V] = sqrt(mv) + bad;
    o[SCVX_FLIGHT_MISS_Q] = sqrt(mq) + bad;
    o[SCVX_FLIGHT_MISS_W] = sqrt(mw) + bad;
    o[SCVX_FLIGHT_MASS_END] = xs[0];
    o[SCVX_FLIGHT_G_MASS] = g_mass + bad;
    o[SCVX_FLIGHT_G_GLIDE] = g_glide + bad;
    o[SCVX_FLIGHT_G_TILT] = g_tilt + bad;
    o[SCVX_FLIGHT_G_RATE] = g_rate + bad;
    o[SCVX_FLIGHT_G_TMAX] = g_tmax;
    o[SCVX_FLIGHT_G_TMIN] = g_tmin;
    o[SCVX_FLIGHT_G_GIMBAL] = g_gimbal;
    o[SCVX_FLIGHT_G_DP] = c.dp ? g_dp + bad : ninf;
    o[SCVX_FLIGHT_G_FIN] = g_fin;
    o[SCVX_FLIGHT_QNORM] = qn + bad;
    if (live) {
        if (flights) {
#pragma unroll
            for (int i = 0; i < SCVX_FLIGHT_NREP; i++) flights[fl * SCVX_FLIGHT_NREP + i] = o[i];
        }
        if (xland) {
#pragma unroll
            for (int i = 0; i < 14; i++) xland[fl * 14 + i] = xs[i];
        }
    }
    // ---- the wavefront's partial row ----
    R* pr = part + ((size_t)b * gridDim.x + blockIdx.x) * MC_NP;
    const bool l0 = threadIdx.x == 0;
#pragma unroll
    for (int i = 0; i < SCVX_FLIGHT_NREP; i++) {
        const R mx = wave_nan_max(live ? o[i] : ninf);
        const R sm = wave_sum(live ? o[i] : R(0.0));
        if (l0) {
            pr[MC_MAX + i] = mx;
            pr[MC_SUM + i] = sm;
        }
    }
    bool any = false;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const bool over = live && o[SCVX_FLIGHT_G_MASS + i] > m.tol;   // a comparison with NaN is false
        any = any || over;
        const int cnt = __popcll(__ballot(over));
        if (l0) pr[MC_CNT + i] = R(cnt);
    }
    {
        const int ca = __popcll(__ballot(any));
        const int cbad = __popcll(__ballot(live && !isfinite(o[SCVX_FLIGHT_GAP])));
        const R lo = wave_sum(live ? R(n_lo) : R(0.0)), hi = wave_sum(live ? R(n_hi) : R(0.0));   // integers below 2^53: exact
        if (l0) {
            pr[MC_ANY] = R(ca);
            pr[MC_BAD] = R(cbad);
            pr[MC_LO] = lo;
            pr[MC_HI] = hi;
        }
    }
    R e[14];
    const R* xK = xb + (size_t)K * 14;
#pragma unroll
    for (int i = 0; i < 14; i++) {
        e[i] = xs[i] - xK[i];
        const R sm = wave_sum(live ? e[i] : R(0.0));
        if (l0) pr[MC_E + i] = sm;
    }
    int t = 0;
#pragma unroll
    for (int i = 0; i < 14; i++) {
#pragma unroll
        for (int j = i; j < 14; j++) {
            const R sm = wave_sum(live ? e[i] * e[j] : R(0.0));
            if (l0) pr[MC_EE + t] = sm;
            t++;
        }
    }
}

// The draws the RNG instantiations consume, written out (scvx_mc_draws_f64): one lane per (plan, s), grid (ceil(S / 64), P); xi0 / xin
// [P][S][14], eta / nud [P][S][K][14] (all 14 columns of a group: nud[.., 0:m] is what a call with m rows reads), each or nullptr.
__global__ __launch_bounds__(64) void mc_draws_kernel(McRngK rg, int S, int K, double* __restrict__ xi0, double* __restrict__ eta,
                                                      double* __restrict__ xin, double* __restrict__ nud) {
    const int p = blockIdx.y;
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= S) return;
    const uint64_t rc2 = mc_rng_c2(rg, p), rc3 = mc_rng_c3(rg, s);
    const size_t fl = (size_t)p * S + s;
    for (int st = 0; st < 2; st++) {
        double* z0 = st == 0 ? xi0 : xin;
        double* zk = st == 0 ? eta : nud;
        const uint64_t c1 = st == 0 ? MC_STREAM_TRUTH : MC_STREAM_NAV;
        if (z0) {
            double z[16];
            mc_draw_group(rg.seed, c1, rc2, rc3, 0, 14, z);
#pragma unroll
            for (int i = 0; i < 14; i++) z0[fl * 14 + i] = z[i];
        }
        if (zk)
            for (int k = 0; k < K; k++) {
                double z[16];
                mc_draw_group(rg.seed, c1, rc2, rc3, 1 + k, 14, z);
#pragma unroll
                for (int i = 0; i < 14; i++) zk[(fl * K + k) * 14 + i] = z[i];
            }
    }
}

// one block per plan: the partial rows of the plan combined in block order, then the report, the mean and the covariance
__global__ __launch_bounds__(256) void mc_finish_kernel(int S, int K, int nblk, const double* __restrict__ part,
                                                        double* __restrict__ mcrep, double* __restrict__ xmean,
                                                        double* __restrict__ xcov) {
    __shared__ double sh[MC_NP];
    const int b = blockIdx.x, t = threadIdx.x;
    const double* pb = part + (size_t)b * nblk * MC_NP;
    if (t < MC_NP) {
        double a = pb[t];
        for (int q = 1; q < nblk; q++) {
            const double v = pb[(size_t)q * MC_NP + t];
            a = t < MC_SUM ? nan_max(a, v) : a + v;
        }
        sh[t] = a;
    }
    __syncthreads();
    const double dS = double(S);
    if (t < SCVX_MC_NREP) {
        double v = 0.0;
        if (t < MC_SUM) v = sh[t];
        else if (t <= MC_ANY) v = sh[t] / dS;
        else if (t == MC_LO || t == MC_HI) v = sh[t] / (dS * double(K));
        else if (t == MC_BAD) v = sh[t];
        else if (t == SCVX_MC_S) v = dS;
        mcrep[(size_t)b * SCVX_MC_NREP + t] = v;
    }
    if (t < 14) xmean[(size_t)b * 14 + t] = sh[MC_E + t] / dS;
    if (t < 196) {
        const int i = t / 14, j = t % 14;
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        const int idx = lo * 14 - (lo * (lo - 1)) / 2 + (hi - lo);
        double v = 0.0;
        if (S > 1) {
            const double mm = sh[MC_E + lo] * sh[MC_E + hi] / dS;
            v = (sh[MC_EE + idx] - mm) / (dS - 1.0);
        }
        xcov[(size_t)b * 196 + t] = v;
    }
}

// the context's workspace of partial rows, grown on demand (hipFree waits for whatever still reads the old one)
hipError_t mc_workspace(scvx_ctx* ctx, size_t doubles) {
    if (ctx->mc_ws_doubles >= doubles) return hipSuccess;
    if (ctx->mc_ws) (void)hipFree(ctx->mc_ws);
    ctx->mc_ws = nullptr;
    ctx->mc_ws_doubles = 0;
    hipError_t e = hipMalloc((void**)&ctx->mc_ws, doubles * 8);
    if (e == hipSuccess) ctx->mc_ws_doubles = doubles;
    return e;
}

hipError_t mc_q_workspace(scvx_ctx* ctx, size_t doubles) {
    if (ctx->mcq_ws_doubles >= doubles) return hipSuccess;
    if (ctx->mcq_ws) (void)hipFree(ctx->mcq_ws);
    ctx->mcq_ws = nullptr;
    ctx->mcq_ws_doubles = 0;
    hipError_t e = hipMalloc((void**)&ctx->mcq_ws, doubles * 8);
    if (e == hipSuccess) ctx->mcq_ws_doubles = doubles;
    return e;
}

void mc_workspace_free(scvx_ctx* ctx) {
    if (ctx->mc_ws) (void)hipFree(ctx->mc_ws);
    ctx->mc_ws = nullptr;
    ctx->mc_ws_doubles = 0;
    if (ctx->mcq_ws) (void)hipFree(ctx->mcq_ws);
    ctx->mcq_ws = nullptr;
    ctx->mcq_ws_doubles = 0;
}

// flights: the caller's dense buffer or nullptr on entry; on return where the flying kernel writes the flights (the workspace when
// only their order statistics are asked for), and pathv likewise (nullptr: the instantiations without per-node samples)
hipError_t mc_q_buffers(scvx_ctx* ctx, int B, int K, int S, const McQ& q, double*& flights, double*& pathv) {
    pathv = q.pathv;
    const size_t nf = (q.flightq && !flights) ? (size_t)B * S * SCVX_FLIGHT_NREP : 0;
    const size_t np = (q.pathq && !q.pathv) ? (size_t)B * (K + 1) * SCVX_PSIG_N * S : 0;
    if (nf + np == 0) return hipSuccess;
    hipError_t e = mc_q_workspace(ctx, nf + np);
    if (e != hipSuccess) return e;
    if (nf) flights = ctx->mcq_ws;
    if (np) pathv = ctx->mcq_ws + nf;
    return hipSuccess;
}

// the order statistics of the sixteen flight columns (rows of S values 16 apart) and of every (b, k, f) row of pathv (contiguous)
hipError_t mc_q_finish(int B, int K, int S, const McQ& q, const double* flights, const double* pathv, hipStream_t st) {
    hipError_t e = hipSuccess;
    if (q.flightq)
        e = launch_order_stats(B * SCVX_FLIGHT_NREP, S, flights, (size_t)S * SCVX_FLIGHT_NREP, SCVX_FLIGHT_NREP, 1, SCVX_FLIGHT_NREP, q.nq,
                               q.ranks, q.flightq, st);
    if (e == hipSuccess && q.pathq)
        e = launch_order_stats(B * (K + 1) * SCVX_PSIG_N, S, pathv, (size_t)S, 1, 0, 1, q.nq, q.ranks, q.pathq, st);
    return e;
}

int check_mc_rng(scvx_ctx* ctx, const scvx_mc_rng* rng) {
    if (!ctx) return SCVX_ERR_ARG;
    if (!rng) return fail(ctx, SCVX_ERR_ARG, "mc rng: null rng");
    if (rng->reserved != 0) return fail(ctx, SCVX_ERR_ARG, "mc rng: reserved must be 0");
    if (rng->independent != 0 && rng->independent != 1) return fail(ctx, SCVX_ERR_ARG, "mc rng: independent must be 0 or 1");
    return SCVX_OK;
}

int check_mc_q(scvx_ctx* ctx, int S, int nq, const int* ranks, const void* flightq, const void* pathq) {
    if (nq == 0 && !flightq && !pathq) return SCVX_OK;   // nothing asked for: the call it extends
    return check_ranks(ctx, S, nq, ranks);
}

hipError_t launch_track_mc(scvx_ctx* ctx, int B, int K, int S, const double* x, const double* u, const double* sigma, const double* gain,
                           const double* C0, const double* xi0, const double* eta, const double* sw, int nsub, int flags, double tol,
                           double* mcrep, double* xmean, double* xcov, double* flights, double* xland, double* dx0, hipStream_t st,
                           const McQ* q, const McRng* rng) {
    const PathK c = path_constants(ctx->prob);
    const double dt = 1.0 / (K + 1);
    const int nblk = (S + 63) / 64;
    hipError_t e = mc_workspace(ctx, (size_t)B * nblk * MC_NP);
    if (e != hipSuccess) return e;
    double* pv = nullptr;
    if (q && (e = mc_q_buffers(ctx, B, K, S, *q, flights, pv)) != hipSuccess) return e;
    McK m{};
    m.tol = tol;
    bool noise = false;
    if ((rng ? rng->noise != 0 : eta != nullptr) && sw)
        for (int i = 0; i < 14; i++) {
            m.sw[i] = sw[i];
            noise = noise || sw[i] > 0.0;
        }
    if (!noise) eta = nullptr;   // sw all zero: the undisturbed kernel path, bit for bit
    const McRngK rg = rng ? mc_rng_k(*rng, noise) : McRngK{};
    const dim3 g((unsigned)nblk, (unsigned)B), blk(64);
    double* part = ctx->mc_ws;
    const DynP<double> dp(ctx->dyn);
#define SCVX_MC_RG(A, F, T, P, G, par)                                                                                                       \
    hipLaunchKernelGGL((mc_fly_kernel<A, F, T, P, G>), g, blk, 0, st, par, c, m, S, K, x, u, sigma, gain, C0, xi0, eta, dt, nsub, flags, part, \
                       flights, xland, dx0, pv, rg)
#define SCVX_MC_PV(A, F, T, P, par)                 \
    do {                                            \
        if (rng) SCVX_MC_RG(A, F, T, P, true, par); \
        else SCVX_MC_RG(A, F, T, P, false, par);    \
    } while (0)
#define SCVX_MC(A, F, T, par)                  \
    do {                                       \
        if (pv) SCVX_MC_PV(A, F, T, true, par); \
        else SCVX_MC_PV(A, F, T, false, par);  \
    } while (0)
    if (ctx->dyn.trq) {
        const DynPT<double> dpt(ctx->dyn);
        if (ctx->dyn.fin) SCVX_MC(true, true, true, dpt);
        else SCVX_MC(true, false, true, dpt);
    } else if (ctx->dyn.fin) {
        if (ctx->dyn.aero) SCVX_MC(true, true, false, dp);
        else SCVX_MC(false, true, false, dp);
    } else if (ctx->dyn.aero)
        SCVX_MC(true, false, false, dp);
    else
        SCVX_MC(false, false, false, dp);
#undef SCVX_MC
#undef SCVX_MC_PV
#undef SCVX_MC_RG
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mc_finish_kernel, dim3((unsigned)B), dim3(256), 0, st, S, K, nblk, part, mcrep, xmean, xcov);
    e = hipGetLastError();
    if (e != hipSuccess || !q) return e;
    return mc_q_finish(B, K, S, *q, flights, pv, st);
}

int check_track_mc(scvx_ctx* ctx, int B, int K, int S, const void* x, const void* u, const void* sigma, const void* gain, const void* C0,
                   const void* xi0, const void* eta, const double* sw, const void* reserved, int nsub, int flags, double tol,
                   const void* mcrep, const void* xmean, const void* xcov) {
    if (!ctx) return SCVX_ERR_ARG;
    if (B < 1 || B > 65535) return fail(ctx, SCVX_ERR_ARG, "track mc: 1 <= B <= 65535 required");
    if (S < 1) return fail(ctx, SCVX_ERR_ARG, "track mc: S >= 1 required");
    if (K != ctx->prob.K) return fail(ctx, SCVX_ERR_ARG, "track mc: K must equal the problem's K");
    if (nsub < 1 || nsub > 1000) return fail(ctx, SCVX_ERR_ARG, "track mc: nsub must be in [1,1000]");
    if (flags & ~SCVX_TRACK_CLAMP) return fail(ctx, SCVX_ERR_ARG, "track mc: unknown flags (SCVX_TRACK_CLAMP)");
    if (!(tol >= 0.0) || !std::isfinite(tol)) return fail(ctx, SCVX_ERR_ARG, "track mc: tol must be finite and >= 0");
    if (sw)
        for (int i = 0; i < 14; i++)
            if (!(sw[i] >= 0.0) || !std::isfinite(sw[i])) return fail(ctx, SCVX_ERR_ARG, "track mc: sw must be finite and >= 0");
    if (eta && !sw) return fail(ctx, SCVX_ERR_ARG, "track mc: eta without sw");
    if (reserved) return fail(ctx, SCVX_ERR_ARG, "track mc: the reserved argument must be NULL");
    if (!x || !u || !sigma || !gain || !C0 || !xi0 || !mcrep || !xmean || !xcov) return fail(ctx, SCVX_ERR_ARG, "track mc: null buffer");
    if (ctx->prob.aero_kind == 1 && !ctx->dyn.aero)
        return fail(ctx, SCVX_ERR_STATE, "AtmosphericData problem: call scvx_set_aero_table first");
    return SCVX_OK;
}

// scvx_track_mc_q_f64 and, with rg (then xi0_dev and eta_dev are placeholders that are never read), scvx_track_mc_rng_f64
static int track_mc_q_dev(scvx_ctx* ctx, int B, int K, int S, const double* x_dev, const double* u_dev, const double* sigma_dev,
                          const double* gain_dev, const double* C0_dev, const double* xi0_dev, const double* eta_dev, const double* sw14,
                          const void* reserved, int nsub, int flags, double tol, double* mcrep_dev, double* xmean_dev, double* xcov_dev,
                          double* flights_dev, double* xland_dev, double* dx0_dev, int nq, const int* ranks, double* flightq_dev,
                          double* pathq_dev, double* pathv_dev, const McRng* rg) {
    int rc = scvx::check_track_mc(ctx, B, K, S, x_dev, u_dev, sigma_dev, gain_dev, C0_dev, xi0_dev, eta_dev, sw14, reserved, nsub, flags,
                                  tol, mcrep_dev, xmean_dev, xcov_dev);
    if (rc) return rc;
    if (rg && (rc = scvx::check_mc_rng(ctx, rg->r))) return rc;
    if ((rc = scvx::check_mc_q(ctx, S, nq, ranks, flightq_dev, pathq_dev))) return rc;
    scvx::McQ q;
    q.nq = nq, q.ranks = ranks, q.flightq = flightq_dev, q.pathq = pathq_dev, q.pathv = pathv_dev;
    const bool any = flightq_dev || pathq_dev || pathv_dev;
    SCVX_HIP(ctx, hipSetDevice(ctx->device));
    SCVX_HIP(ctx, scvx::launch_track_mc(ctx, B, K, S, x_dev, u_dev, sigma_dev, gain_dev, C0_dev, rg ? nullptr : xi0_dev,
                                        rg ? nullptr : eta_dev, sw14, nsub, flags, tol, mcrep_dev, xmean_dev, xcov_dev, flights_dev,
                                        xland_dev, dx0_dev, ctx->stream, any ? &q : nullptr, rg));
    return SCVX_OK;
}

// scvx_track_mc_q_f64_host and, with rg (xi0 and eta placeholders, nothing of them uploaded), scvx_track_mc_rng_f64_host
static int track_mc_q_host(scvx_ctx* ctx, int B, int K, int S, const double* x, const double* u, const double* sigma, const double* gain,
                           const double* C0, const double* xi0, const double* eta, const double* sw14, const void* reserved, int nsub,
                           int flags, double tol, double* mcrep, double* xmean, double* xcov, double* flights, double* xland, double* dx0,
                           int nq, const int* ranks, double* flightq, double* pathq, double* pathv, const McRng* rg);

// one lane per (plan, s): the draws the _rng forms consume (mc_draws_kernel); any of the four outputs may be nullptr
hipError_t launch_mc_draws(const scvx_mc_rng& r, int P, int S, int K, double* xi0, double* eta, double* xin, double* nud, hipStream_t st) {
    const McRng g{&r, 0};
    hipLaunchKernelGGL(mc_draws_kernel, dim3((unsigned)((S + 63) / 64), (unsigned)P), dim3(64), 0, st, mc_rng_k(g, false), S, K, xi0, eta,
                       xin, nud);
    return hipGetLastError();
}

int check_mc_draws(scvx_ctx* ctx, const scvx_mc_rng* rng, int P, int S, int K) {
    int rc = check_mc_rng(ctx, rng);
    if (rc) return rc;
    if (P < 1 || P > 65535) return fail(ctx, SCVX_ERR_ARG, "mc draws: 1 <= P <= 65535 required");
    if (S < 1) return fail(ctx, SCVX_ERR_ARG, "mc draws: S >= 1 required");
    if (K < 1) return fail(ctx, SCVX_ERR_ARG, "mc draws: K >= 1 required");
    return SCVX_OK;
}

}  // namespace scvx

extern "C" {

int scvx_mc_draws_f64(scvx_ctx* ctx, const scvx_mc_rng* rng, int P, int S, int K, double* xi0_dev, double* eta_dev, double* xin_dev,
                      double* nud_dev) {
    int rc = scvx::check_mc_draws(ctx, rng, P, S, K);
    if (rc) return rc;
    SCVX_HIP(ctx, hipSetDevice(ctx->device));
    SCVX_HIP(ctx, scvx::launch_mc_draws(*rng, P, S, K, xi0_dev, eta_dev, xin_dev, nud_dev, ctx->stream));
    return SCVX_OK;
}

int scvx_mc_draws_f64_host(scvx_ctx* ctx, const scvx_mc_rng* rng, int P, int S, int K, double* xi0, double* eta, double* xin, double* nud) {
    int rc = scvx::check_mc_draws(ctx, rng, P, S, K);
    if (rc) return rc;
    SCVX_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n0 = (size_t)P * S * 14, nk = n0 * K;
    scvx::DevBuf<double> d0, d1, d2, d3;
    if (xi0) SCVX_HIP(ctx, hipMalloc((void**)&d0.p, n0 * 8));
    if (eta) SCVX_HIP(ctx, hipMalloc((void**)&d1.p, nk * 8));
    if (xin) SCVX_HIP(ctx, hipMalloc((void**)&d2.p, n0 * 8));
    if (nud) SCVX_HIP(ctx, hipMalloc((void**)&d3.p, nk * 8));
    hipStream_t st = ctx->stream;
    SCVX_HIP(ctx, scvx::launch_mc_draws(*rng, P, S, K, d0.p, d1.p, d2.p, d3.p, st));
    if (xi0) SCVX_HIP(ctx, hipMemcpyAsync(xi0, d0.p, n0 * 8, hipMemcpyDeviceToHost, st));
    if (eta) SCVX_HIP(ctx, hipMemcpyAsync(eta, d1.p, nk * 8, hipMemcpyDeviceToHost, st));
    if (xin) SCVX_HIP(ctx, hipMemcpyAsync(xin, d2.p, n0 * 8, hipMemcpyDeviceToHost, st));
    if (nud) SCVX_HIP(ctx, hipMemcpyAsync(nud, d3.p, nk * 8, hipMemcpyDeviceToHost, st));
    SCVX_HIP(ctx, hipStreamSynchronize(st));
    return SCVX_OK;
}

int scvx_track_mc_q_f64(scvx_ctx* ctx, int B, int K, int S, const double* x_dev, const double* u_dev, const double* sigma_dev,
                        const double* gain_dev, const double* C0_dev, const double* xi0_dev, const double* eta_dev, const double* sw14,
                        const void* reserved, int nsub, int flags, double tol, double* mcrep_dev, double* xmean_dev, double* xcov_dev,
                        double* flights_dev, double* xland_dev, double* dx0_dev, int nq, const int* ranks, double* flightq_dev,
                        double* pathq_dev, double* pathv_dev) {
    return scvx::track_mc_q_dev(ctx, B, K, S, x_dev, u_dev, sigma_dev, gain_dev, C0_dev, xi0_dev, eta_dev, sw14, reserved, nsub, flags, tol,
                                mcrep_dev, xmean_dev, xcov_dev, flights_dev, xland_dev, dx0_dev, nq, ranks, flightq_dev, pathq_dev,
                                pathv_dev, nullptr);
}

// the placeholders: xi0 any non-null pointer, eta non-null exactly when the truth receives impulses (check_track_mc's rules for them)
int scvx_track_mc_rng_f64(scvx_ctx* ctx, int B, int K, int S, const double* x_dev, const double* u_dev, const double* sigma_dev,
                          const double* gain_dev, const double* C0_dev, const scvx_mc_rng* rng, int noise, const double* sw14,
                          const void* reserved, int nsub, int flags, double tol, double* mcrep_dev, double* xmean_dev, double* xcov_dev,
                          double* flights_dev, double* xland_dev, double* dx0_dev, int nq, const int* ranks, double* flightq_dev,
                          double* pathq_dev, double* pathv_dev) {
    const scvx::McRng rg{rng, noise};
    return scvx::track_mc_q_dev(ctx, B, K, S, x_dev, u_dev, sigma_dev, gain_dev, C0_dev, x_dev, noise ? x_dev : nullptr, sw14, reserved,
                                nsub, flags, tol, mcrep_dev, xmean_dev, xcov_dev, flights_dev, xland_dev, dx0_dev, nq, ranks, flightq_dev,
                                pathq_dev, pathv_dev, &rg);
}

int scvx_track_mc_rng_f64_host(scvx_ctx* ctx, int B, int K, int S, const double* x, const double* u, const double* sigma,
                               const double* gain, const double* C0, const scvx_mc_rng* rng, int noise, const double* sw14,
                               const void* reserved, int nsub, int flags, double tol, double* mcrep, double* xmean, double* xcov,
                               double* flights, double* xland, double* dx0, int nq, const int* ranks, double* flightq, double* pathq,
                               double* pathv) {
    const scvx::McRng rg{rng, noise};
    return scvx::track_mc_q_host(ctx, B, K, S, x, u, sigma, gain, C0, x, noise ? x : nullptr, sw14, reserved, nsub, flags, tol, mcrep,
                                 xmean, xcov, flights, xland, dx0, nq, ranks, flightq, pathq, pathv, &rg);
}

int scvx_track_mc_f64(scvx_ctx* ctx, int B, int K, int S, const double* x_dev, const double* u_dev, const double* sigma_dev,
                      const double* gain_dev, const double* C0_dev, const double* xi0_dev, const double* eta_dev, const double* sw14,
                      const void* reserved, int nsub, int flags, double tol, double* mcrep_dev, double* xmean_dev, double* xcov_dev,
                      double* flights_dev, double* xland_dev, double* dx0_dev) {
    return scvx_track_mc_q_f64(ctx, B, K, S, x_dev, u_dev, sigma_dev, gain_dev, C0_dev, xi0_dev, eta_dev, sw14, reserved, nsub, flags, tol,
                               mcrep_dev, xmean_dev, xcov_dev, flights_dev, xland_dev, dx0_dev, 0, nullptr, nullptr, nullptr, nullptr);
}

int scvx_track_mc_f64_host(scvx_ctx* ctx, int B, int K, int S, const double* x, const double* u, const double* sigma, const double* gain,
                           const double* C0, const double* xi0, const double* eta, const double* sw14, const void* reserved, int nsub,
                           int flags, double tol, double* mcrep, double* xmean, double* xcov, double* flights, double* xland,
                           double* dx0) {
    return scvx_track_mc_q_f64_host(ctx, B, K, S, x, u, sigma, gain, C0, xi0, eta, sw14, reserved, nsub, flags, tol, mcrep, xmean, xcov,
                                    flights, xland, dx0, 0, nullptr, nullptr, nullptr, nullptr);
}

int scvx_track_mc_q_f64_host(scvx_ctx* ctx, int B, int K, int S, const double* x, const double* u, const double* sigma,
                             const double* gain, const double* C0, const double* xi0, const double* eta, const double* sw14,
                             const void* reserved, int nsub, int flags, double tol, double* mcrep, double* xmean, double* xcov,
                             double* flights, double* xland, double* dx0, int nq, const int* ranks, double* flightq, double* pathq,
                             double* pathv) {
    return scvx::track_mc_q_host(ctx, B, K, S, x, u, sigma, gain, C0, xi0, eta, sw14, reserved, nsub, flags, tol, mcrep, xmean, xcov,
                                 flights, xland, dx0, nq, ranks, flightq, pathq, pathv, nullptr);
}

}  // extern "C"

namespace scvx {

static int track_mc_q_host(scvx_ctx* ctx, int B, int K, int S, const double* x, const double* u, const double* sigma, const double* gain,
                           const double* C0, const double* xi0, const double* eta, const double* sw14, const void* reserved, int nsub,
                           int flags, double tol, double* mcrep, double* xmean, double* xcov, double* flights, double* xland, double* dx0,
                           int nq, const int* ranks, double* flightq, double* pathq, double* pathv, const McRng* rg) {
    int rc = scvx::check_track_mc(ctx, B, K, S, x, u, sigma, gain, C0, xi0, eta, sw14, reserved, nsub, flags, tol, mcrep, xmean, xcov);
    if (rc) return rc;
    if (rg && (rc = scvx::check_mc_rng(ctx, rg->r))) return rc;
    if (rg) xi0 = eta = nullptr;   // placeholders until here: the lanes make the draws
    if ((rc = scvx::check_mc_q(ctx, S, nq, ranks, flightq, pathq))) return rc;
    SCVX_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nfq = (size_t)B * SCVX_FLIGHT_NREP * nq, npq = (size_t)B * (K + 1) * SCVX_PSIG_N * nq,
                 npv = (size_t)B * (K + 1) * SCVX_PSIG_N * S;
    scvx::DevBuf<double> dfq, dpq, dpv;
    if (flightq) SCVX_HIP(ctx, hipMalloc((void**)&dfq.p, nfq * 8));
    if (pathq) SCVX_HIP(ctx, hipMalloc((void**)&dpq.p, npq * 8));
    if (pathv) SCVX_HIP(ctx, hipMalloc((void**)&dpv.p, npv * 8));
    scvx::McQ q;
    q.nq = nq, q.ranks = ranks, q.flightq = dfq.p, q.pathq = dpq.p, q.pathv = dpv.p;
    const bool any = flightq || pathq || pathv;
    const int NU = scvx_control_dim(ctx), n = 14 + NU;
    const size_t nx = (size_t)B * (K + 1) * 14, nu = (size_t)B * (K + 1) * NU, ng = (size_t)B * K * NU * n, nc = (size_t)B * 196,
                 ni = (size_t)S * 14, ne = (size_t)S * K * 14, nr = (size_t)B * SCVX_MC_NREP, nm = (size_t)B * 14,
                 nf = (size_t)B * S * SCVX_FLIGHT_NREP, nl = (size_t)B * S * 14;
    scvx::DevBuf<double> dx, du, ds, dg, dc, di, de, dr, dm, dv, df, dl, d0;
    SCVX_HIP(ctx, hipMalloc((void**)&dx.p, nx * 8));
    SCVX_HIP(ctx, hipMalloc((void**)&du.p, nu * 8));
    SCVX_HIP(ctx, hipMalloc((void**)&ds.p, (size_t)B * 8));
    SCVX_HIP(ctx, hipMalloc((void**)&dg.p, ng * 8));
    SCVX_HIP(ctx, hipMalloc((void**)&dc.p, nc * 8));
    if (xi0) SCVX_HIP(ctx, hipMalloc((void**)&di.p, ni * 8));
    if (eta) SCVX_HIP(ctx, hipMalloc((void**)&de.p, ne * 8));
    SCVX_HIP(ctx, hipMalloc((void**)&dr.p, nr * 8));
    SCVX_HIP(ctx, hipMalloc((void**)&dm.p, nm * 8));
    SCVX_HIP(ctx, hipMalloc((void**)&dv.p, nc * 8));
    if (flights) SCVX_HIP(ctx, hipMalloc((void**)&df.p, nf * 8));
    if (xland) SCVX_HIP(ctx, hipMalloc((void**)&dl.p, nl * 8));
    if (dx0) SCVX_HIP(ctx, hipMalloc((void**)&d0.p, nl * 8));
    hipStream_t st = ctx->stream;
    SCVX_HIP(ctx, hipMemcpyAsync(dx.p, x, nx * 8, hipMemcpyHostToDevice, st));
    SCVX_HIP(ctx, hipMemcpyAsync(du.p, u, nu * 8, hipMemcpyHostToDevice, st));
    SCVX_HIP(ctx, hipMemcpyAsync(ds.p, sigma, (size_t)B * 8, hipMemcpyHostToDevice, st));
    SCVX_HIP(ctx, hipMemcpyAsync(dg.p, gain, ng * 8, hipMemcpyHostToDevice, st));
    SCVX_HIP(ctx, hipMemcpyAsync(dc.p, C0, nc * 8, hipMemcpyHostToDevice, st));
    if (xi0) SCVX_HIP(ctx, hipMemcpyAsync(di.p, xi0, ni * 8, hipMemcpyHostToDevice, st));
    if (eta) SCVX_HIP(ctx, hipMemcpyAsync(de.p, eta, ne * 8, hipMemcpyHostToDevice, st));
    SCVX_HIP(ctx, scvx::launch_track_mc(ctx, B, K, S, dx.p, du.p, ds.p, dg.p, dc.p, di.p, de.p, sw14, nsub, flags, tol, dr.p, dm.p, dv.p,
                                        df.p, dl.p, d0.p, st, any ? &q : nullptr, rg));
    if (flightq) SCVX_HIP(ctx, hipMemcpyAsync(flightq, dfq.p, nfq * 8, hipMemcpyDeviceToHost, st));
    if (pathq) SCVX_HIP(ctx, hipMemcpyAsync(pathq, dpq.p, npq * 8, hipMemcpyDeviceToHost, st));
    if (pathv) SCVX_HIP(ctx, hipMemcpyAsync(pathv, dpv.p, npv * 8, hipMemcpyDeviceToHost, st));
    SCVX_HIP(ctx, hipMemcpyAsync(mcrep, dr.p, nr * 8, hipMemcpyDeviceToHost, st));
    SCVX_HIP(ctx, hipMemcpyAsync(xmean, dm.p, nm * 8, hipMemcpyDeviceToHost, st));
    SCVX_HIP(ctx, hipMemcpyAsync(xcov, dv.p, nc * 8, hipMemcpyDeviceToHost, st));
    if (flights) SCVX_HIP(ctx, hipMemcpyAsync(flights, df.p, nf * 8, hipMemcpyDeviceToHost, st));
    if (xland) SCVX_HIP(ctx, hipMemcpyAsync(xland, dl.p, nl * 8, hipMemcpyDeviceToHost, st));
    if (dx0) SCVX_HIP(ctx, hipMemcpyAsync(dx0, d0.p, nl * 8, hipMemcpyDeviceToHost, st));
    SCVX_HIP(ctx, hipStreamSynchronize(st));
    return SCVX_OK;
}

}  // namespace scvx
