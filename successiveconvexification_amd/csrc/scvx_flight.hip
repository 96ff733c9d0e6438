// The walk of a plan (scvx_flight_check_f64, scvx_track_fly_f64, include/scvx.h): the rollout of a batch of plans, open loop or under
// the tracking law of scvx_track.hip, and the audit of their path constraints between the nodes.  No counterpart in the reference,
// which imposes every path constraint of build_model (rocketland.jl:136-209) at the nodes and never re-flies a plan.
//
// fly_kernel: ONE LANE PER TRAJECTORY.  The K segments of a trajectory depend on each other (single shooting), so the lane
// walks its K x nsub RK4 substeps in order with the arithmetic of propagate_kernel (scvx_discretize.hip: rhs_only<>, first-order
// hold from the two node values, the same fma forms, sigma scaling).  At every substep boundary s = 0..nsub of every segment it
// evaluates the path functions and keeps their running maxima in registers; nothing but the K+1 node rows (optional) and the
// 16-double report leaves the lane.  Blocks of one wavefront: at B = 8,192 that is 128 wavefronts over 256 CUs, each alone on
// its SIMD -- the walk is one long dependent chain, so wavefronts are spread, not stacked.  Constants ride by value in the kernel
// argument (scalar registers), as DynPK does; no LDS.
//
// TRACK = false is the flight check: the next node's control is the planned one, and in PLAN mode the state restarts from the plan
// at every node.  TRACK = true is the closed-loop flight: the feedback u_{k+1} = ubar_{k+1} + L_k [x_k - xbar_k; u_k - ubar_k] is
// formed at every node from the FLOWN state and the APPLIED control, with an optional clamp of the commanded thrust / fin norms and
// an initial state offset per trajectory.  Everything else is written once, in one kernel body specialised by the constant TRACK:
// each instantiation compiles to what a kernel of its own compiled to (profiles/fly_kernel_merge.md).  The substep is a copy of
// propagate_kernel's, not a function shared with it: lifted into one, it is contracted and allocated differently in every kernel.
//
// NAV = one trailing pointer (scvx_track_fly_nav_f64): the law is fed a navigation estimate, z = [(x - nav_k) - xbar_k; u_k - ubar_k]
// with nav [B][K][14] the estimate's error at node k.  It is a parameter PACK, empty in every other instantiation, so that those
// keep their kernel argument and their registers exactly (profiles/nav.md).
#include <cmath>
#include <limits>
#include "scvx_internal.hpp"

namespace scvx {

PathK path_constants(const scvx_problem& P) {
    const double d2r = M_PI / 180.0;
    PathK c{};
    for (int i = 0; i < 3; i++) { c.rIf[i] = P.rIf[i]; c.vIf[i] = P.vIf[i]; c.wBf[i] = P.wBf[i]; }
    for (int i = 0; i < 4; i++) c.qBIf[i] = P.qBIf[i];
    c.mdry = P.mdry;
    c.tggs = std::tan(P.gammaGs * d2r);
    c.sqcm = std::sqrt((1.0 - std::cos(P.thetaMax * d2r)) / 2.0);
    c.omMax = P.omMax;
    c.Tmax = P.Tmax;
    c.Tmin = P.Tmin;
    c.inv_cosd = 1.0 / std::cos(P.deltaMax * d2r);
    c.dp = (P.model_flags & SCVX_MODEL_DPMAX) ? 1 : 0;
    c.vmax = c.dp ? std::sqrt(2.0 * P.dpMax / P.rho) : 0.0;
    c.finmxf = P.finmxf;
    return c;
}

// opt: the mode (SCVX_FLIGHT_SHOOT / PLAN) of the flight check, the flags (SCVX_TRACK_CLAMP) of the closed-loop flight;
// gain, dx0 and ufly are read only with TRACK
template <class... P>
__device__ __forceinline__ const double* fly_nav(P... p) {
    if constexpr (sizeof...(P) > 0) return (p, ...);
    else return nullptr;
}

template <bool AERO, bool FIN, bool TRQ, bool TRACK, class... NAV>
__global__ __launch_bounds__(64) void fly_kernel(DynPK<double, TRQ> p, PathK c, int B, int K, const double* __restrict__ x,
                                                 const double* __restrict__ u, const double* __restrict__ sigma,
                                                 const double* __restrict__ gain, const double* __restrict__ dx0, double dt, int nsub,
                                                 int opt, double* __restrict__ report, double* __restrict__ xfly,
                                                 double* __restrict__ ufly, NAV... nav) {
    static_assert(sizeof...(NAV) == 0 || TRACK, "a navigation estimate feeds the tracking law");
    typedef double R;
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    constexpr int NU = FIN ? 5 : 3;
    constexpr int n = 14 + NU;
    const R* xb = x + (size_t)b * (K + 1) * 14;
    const R* ub = u + (size_t)b * (K + 1) * NU;
    const R* gb = TRACK ? gain + (size_t)b * K * NU * n : nullptr;
    R* xf = xfly ? xfly + (size_t)b * (K + 1) * 14 : nullptr;
    R* uf = (TRACK && ufly) ? ufly + (size_t)b * (K + 1) * NU : nullptr;
    const R sig = sigma[b];
    const R h = dt / R(nsub);
    const R inv_n = R(1.0) / R(nsub);
    const R ninf = -std::numeric_limits<double>::infinity();
    const bool clamp = TRACK && (opt & SCVX_TRACK_CLAMP) != 0;
    R xs[14], ukv[NU], upv[NU];
#pragma unroll
    for (int i = 0; i < 14; i++) xs[i] = xb[i];
    if (TRACK && dx0) {
#pragma unroll
        for (int i = 0; i < 14; i++) xs[i] += dx0[(size_t)b * 14 + i];
    }
#pragma unroll
    for (int j = 0; j < NU; j++) upv[j] = ub[j];
    if (xf) {
#pragma unroll
        for (int i = 0; i < 14; i++) xf[i] = xs[i];
    }
    if (uf) {
#pragma unroll
        for (int j = 0; j < NU; j++) uf[j] = upv[j];
    }
    R gap = R(0.0), bad = R(0.0);   // bad: 0 while every sampled state (and every node difference) is finite, else NaN
    R g_mass = ninf, g_glide = ninf, g_tilt = ninf, g_rate = ninf, g_tmax = ninf, g_tmin = ninf, g_gimbal = ninf, g_dp = ninf,
      g_fin = ninf, qn = R(0.0);
    for (int k = 0; k < K; k++) {
        if constexpr (TRACK) {
            // ---- node k: the next node's control from the flown state and the applied control ----
            R z[n];
#pragma unroll
            for (int i = 0; i < 14; i++) {
                if constexpr (sizeof...(NAV) > 0) z[i] = (xs[i] - fly_nav(nav...)[((size_t)b * K + k) * 14 + i]) - xb[(size_t)k * 14 + i];
                else z[i] = xs[i] - xb[(size_t)k * 14 + i];
            }
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
            if (uf) {
#pragma unroll
                for (int j = 0; j < NU; j++) uf[(size_t)(k + 1) * NU + j] = upv[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < NU; j++) { ukv[j] = upv[j]; upv[j] = ub[(size_t)(k + 1) * NU + j]; }
            if (opt == SCVX_FLIGHT_PLAN && k > 0) {
#pragma unroll
                for (int i = 0; i < 14; i++) xs[i] = xb[(size_t)k * 14 + i];
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
        // ---- node k + 1: the flown state against the planned one ----
        const R* xn = xb + (size_t)(k + 1) * 14;
#pragma unroll
        for (int i = 0; i < 14; i++) {
            const R d = xs[i] - xn[i];
            gap = nan_max(gap, fabs(d));
            bad = fma(d, R(0.0), bad);
        }
        if (xf) {
#pragma unroll
            for (int i = 0; i < 14; i++) xf[(size_t)(k + 1) * 14 + i] = xs[i];
        }
    }
    // xs is the flown final node (in PLAN mode: the end of the last segment)
    R mr = R(0.0), mv = R(0.0), mq = R(0.0), mw = R(0.0);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const R dr = xs[1 + i] - c.rIf[i], dv = xs[4 + i] - c.vIf[i], dw = xs[11 + i] - c.wBf[i];
        mr = fma(dr, dr, mr); mv = fma(dv, dv, mv); mw = fma(dw, dw, mw);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) { const R dq = xs[7 + i] - c.qBIf[i]; mq = fma(dq, dq, mq); }
    R* o = report + (size_t)b * SCVX_FLIGHT_NREP;
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
}

template <bool TRACK, class... NAV>
static hipError_t launch_fly(const scvx_ctx* ctx, int B, int K, const double* x, const double* u, const double* sigma, const double* gain,
                             const double* dx0, int nsub, int opt, double* report, double* xfly, double* ufly, hipStream_t st,
                             NAV... nav) {
    const PathK c = path_constants(ctx->prob);
    const double dt = 1.0 / (K + 1);
    const dim3 g((unsigned)((B + 63) / 64)), blk(64);
    const DynP<double> dp(ctx->dyn);
#define SCVX_FLY(A, F, T, par) \
    hipLaunchKernelGGL((fly_kernel<A, F, T, TRACK, NAV...>), g, blk, 0, st, par, c, B, K, x, u, sigma, gain, dx0, dt, nsub, opt, report, \
                       xfly, ufly, nav...)
    if (ctx->dyn.trq) {
        const DynPT<double> dpt(ctx->dyn);
        if (ctx->dyn.fin) SCVX_FLY(true, true, true, dpt);
        else SCVX_FLY(true, false, true, dpt);
    } else if (ctx->dyn.fin) {
        if (ctx->dyn.aero) SCVX_FLY(true, true, false, dp);
        else SCVX_FLY(false, true, false, dp);
    } else if (ctx->dyn.aero)
        SCVX_FLY(true, false, false, dp);
    else
        SCVX_FLY(false, false, false, dp);
#undef SCVX_FLY
    return hipGetLastError();
}

hipError_t launch_flight(const scvx_ctx* ctx, int B, int K, const double* x, const double* u, const double* sigma, int nsub,
                         int mode, double* report, double* xfly, hipStream_t st) {
    return launch_fly<false>(ctx, B, K, x, u, sigma, nullptr, nullptr, nsub, mode, report, xfly, nullptr, st);
}

hipError_t launch_track_fly(const scvx_ctx* ctx, int B, int K, const double* x, const double* u, const double* sigma, const double* gain,
                            const double* dx0, int nsub, int flags, double* report, double* xfly, double* ufly, hipStream_t st) {
    return launch_fly<true>(ctx, B, K, x, u, sigma, gain, dx0, nsub, flags, report, xfly, ufly, st);
}

hipError_t launch_track_fly_nav(const scvx_ctx* ctx, int B, int K, const double* x, const double* u, const double* sigma,
                                const double* gain, const double* dx0, const double* nav, int nsub, int flags, double* report,
                                double* xfly, double* ufly, hipStream_t st) {
    return launch_fly<true>(ctx, B, K, x, u, sigma, gain, dx0, nsub, flags, report, xfly, ufly, st, nav);
}

}  // namespace scvx
