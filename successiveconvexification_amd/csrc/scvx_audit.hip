// The segment audit (scvx_segment_audit_f64, scvx_batch_segment_audit, scvx_batch_audit_margins, include/scvx.h): the PLAN-mode flight
// check taken apart.  In PLAN mode the state restarts at every planned node, so the K segments of a plan do not depend on each other;
// fly_kernel (scvx_flight.hip) nevertheless walks them as one chain on one lane and keeps one maximum per column over the whole flight.
// Here every segment is a lane of its own and keeps its own maxima: where a constraint fails between the nodes leaves the device, and
// the dependent chain is K times shorter.  No counterpart in the reference, which imposes every path constraint at the nodes.
//
// audit_kernel: ONE LANE PER (b, k), consecutive lanes on consecutive k -- K2's parallelisation (propagate_kernel, scvx_discretize.hip)
// with the path functions of fly_kernel sampled at the nsub + 1 substep boundaries.  The substep is a copy of propagate_kernel's /
// fly_kernel's, statement for statement, not a function shared with them (see the header of scvx_flight.hip), and the samples are
// fly_kernel's expressions with nan_max.  `bad` is the segment's own: a non-finite sampled state makes the state columns of THAT segment
// NaN.  (A non-finite node k is the start of segment k and the node the end of segment k - 1 is compared with: segment k - 1 shows it
// in its DEFECT alone.)  Blocks of one wavefront, so that B K / 64 wavefronts spread over the CUs rather than stack on a few; constants
// by value in the kernel argument (scalar registers); no LDS.
//
// audit_report_kernel: the PLAN-mode report [B][SCVX_FLIGHT_NREP] from seg, one wavefront per plan: lane l takes segments l, l + 64, ..
// in order, then a butterfly over the lanes -- a fixed order, so two launches agree bit for bit.  The miss columns and MASS_END are
// those of the last segment's end, which audit_kernel left in the report's row.
//
// audit_margins_kernel: the back-offs of scvx_batch_audit_margins from seg, one block per plan, on the pattern of
// margins_from_psig_kernel (scvx_batch.hip).
#include <cmath>
#include <limits>
#include "scvx_internal.hpp"
#include "scvx_stage.hpp"

namespace scvx {

template <bool AERO, bool FIN, bool TRQ>
__global__ __launch_bounds__(64) void audit_kernel(DynPK<double, TRQ> p, PathK c, long nseg, int K, const double* __restrict__ x,
                                                   const double* __restrict__ u, const double* __restrict__ sigma, double dt, int nsub,
                                                   double* __restrict__ segs, double* __restrict__ report) {
    typedef double R;
    const long seg = (long)blockIdx.x * 64 + threadIdx.x;
    if (seg >= nseg) return;
    const long b = seg / K;
    const int k = (int)(seg - b * K);
    constexpr int NU = FIN ? 5 : 3;
    const R* xk = x + ((size_t)b * (K + 1) + k) * 14;
    const R* uk = u + ((size_t)b * (K + 1) + k) * NU;
    const R sig = sigma[b];
    const R h = dt / R(nsub);
    const R inv_n = R(1.0) / R(nsub);
    const R ninf = -std::numeric_limits<double>::infinity();
    R xs[14], ukv[NU], upv[NU];
#pragma unroll
    for (int i = 0; i < 14; i++) xs[i] = xk[i];
#pragma unroll
    for (int j = 0; j < NU; j++) { ukv[j] = uk[j]; upv[j] = uk[NU + j]; }
    R gap = R(0.0), bad = R(0.0);   // bad: 0 while every sampled state of this segment is finite, else NaN
    R g_mass = ninf, g_glide = ninf, g_tilt = ninf, g_rate = ninf, g_tmax = ninf, g_tmin = ninf, g_gimbal = ninf, g_dp = ninf,
      g_fin = ninf, qn = R(0.0);
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
    // ---- node k + 1: the end of the segment against the planned node ----
    const R* xn = xk + 14;
#pragma unroll
    for (int i = 0; i < 14; i++) gap = nan_max(gap, fabs(xs[i] - xn[i]));
    R* o = segs + (size_t)seg * SCVX_SEG_N;
    o[SCVX_SEG_DEFECT] = gap + bad;
    o[SCVX_SEG_G_MASS] = g_mass + bad;
    o[SCVX_SEG_G_GLIDE] = g_glide + bad;
    o[SCVX_SEG_G_TILT] = g_tilt + bad;
    o[SCVX_SEG_G_RATE] = g_rate + bad;
    o[SCVX_SEG_G_TMAX] = g_tmax;
    o[SCVX_SEG_G_TMIN] = g_tmin;
    o[SCVX_SEG_G_GIMBAL] = g_gimbal;
    o[SCVX_SEG_G_DP] = c.dp ? g_dp + bad : ninf;
    o[SCVX_SEG_G_FIN] = g_fin;
    o[SCVX_SEG_QNORM] = qn + bad;
    if (report && k == K - 1) {
        // xs is the end of the last segment: what the PLAN-mode flight check measures its misses on
        R mr = R(0.0), mv = R(0.0), mq = R(0.0), mw = R(0.0);
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const R dr = xs[1 + i] - c.rIf[i], dv = xs[4 + i] - c.vIf[i], dw = xs[11 + i] - c.wBf[i];
            mr = fma(dr, dr, mr); mv = fma(dv, dv, mv); mw = fma(dw, dw, mw);
        }
#pragma unroll
        for (int i = 0; i < 4; i++) { const R dq = xs[7 + i] - c.qBIf[i]; mq = fma(dq, dq, mq); }
        R* r = report + (size_t)b * SCVX_FLIGHT_NREP;
        r[SCVX_FLIGHT_MISS_R] = sqrt(mr);
        r[SCVX_FLIGHT_MISS_V] = sqrt(mv);
        r[SCVX_FLIGHT_MISS_Q] = sqrt(mq);
        r[SCVX_FLIGHT_MISS_W] = sqrt(mw);
        r[SCVX_FLIGHT_MASS_END] = xs[0];
    }
}

// the report's column of a seg column: DEFECT is the report's GAP, the rest keep the report's order
static_assert(SCVX_SEG_G_MASS + 5 == SCVX_FLIGHT_G_MASS && SCVX_SEG_QNORM + 5 == SCVX_FLIGHT_QNORM && SCVX_SEG_DEFECT == SCVX_FLIGHT_GAP,
              "seg keeps the flight report's order");
__device__ __forceinline__ constexpr int audit_rep_col(int c) { return c == SCVX_SEG_DEFECT ? SCVX_FLIGHT_GAP : c + 5; }

__global__ __launch_bounds__(64) void audit_report_kernel(int B, int K, const double* __restrict__ segs, double* __restrict__ report) {
    const int b = blockIdx.x;
    if (b >= B) return;
    const double* s = segs + (size_t)b * K * SCVX_SEG_N;
    double m[SCVX_SEG_N];
#pragma unroll
    for (int c = 0; c < SCVX_SEG_N; c++) m[c] = -std::numeric_limits<double>::infinity();
    for (int k = threadIdx.x; k < K; k += 64) {
#pragma unroll
        for (int c = 0; c < SCVX_SEG_N; c++) m[c] = nan_max(m[c], s[(size_t)k * SCVX_SEG_N + c]);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int c = 0; c < SCVX_SEG_N; c++) m[c] = nan_max(m[c], __shfl_xor(m[c], off, 64));
    }
    if (threadIdx.x != 0) return;
    double* r = report + (size_t)b * SCVX_FLIGHT_NREP;
#pragma unroll
    for (int c = 0; c < SCVX_SEG_N; c++) r[audit_rep_col(c)] = m[c];
    // a non-finite state anywhere in the plan makes its misses NaN, as the flight check's do (its GAP is NaN then)
    const double bad = fma(m[SCVX_SEG_DEFECT], 0.0, 0.0);
    r[SCVX_FLIGHT_MISS_R] += bad;
    r[SCVX_FLIGHT_MISS_V] += bad;
    r[SCVX_FLIGHT_MISS_Q] += bad;
    r[SCVX_FLIGHT_MISS_W] += bad;
}

// e_k = max(excess(k - 1), excess(k)) of column col of seg [K][SCVX_SEG_N]; excess = G where G > tol, else 0
__device__ __forceinline__ double audit_excess(const double* s, int K, int k, int col, double tol) {
    double e = 0.0;
    if (k > 0) { const double g = s[(size_t)(k - 1) * SCVX_SEG_N + col]; if (g > tol) e = g; }
    if (k < K) { const double g = s[(size_t)k * SCVX_SEG_N + col]; if (g > tol) e = fmax(e, g); }
    return e;
}

__global__ __launch_bounds__(64) void audit_margins_kernel(int B, int K, const double* __restrict__ segs, const double* __restrict__ x,
                                                           double gain, double tol, AuditCaps capw, unsigned which,
                                                           double* __restrict__ marg, double* __restrict__ pmarg) {
    const int b = blockIdx.x;
    if (b >= B) return;
    const double* s = segs + (size_t)b * K * SCVX_SEG_N;
    int bad = 0;
    for (int k = threadIdx.x; k < K; k += 64) {
        const double* g = s + (size_t)k * SCVX_SEG_N;
        bad |= (which & SCVX_MARGIN_THRUST) && !(g[SCVX_SEG_G_TMIN] == g[SCVX_SEG_G_TMIN]);
        bad |= (which & SCVX_MARGIN_GLIDE) && !(g[SCVX_SEG_G_GLIDE] == g[SCVX_SEG_G_GLIDE]);
        bad |= (which & SCVX_MARGIN_TILT) && !(g[SCVX_SEG_G_TILT] == g[SCVX_SEG_G_TILT]);
        bad |= (which & SCVX_MARGIN_RATE) && !(g[SCVX_SEG_G_RATE] == g[SCVX_SEG_G_RATE]);
    }
    if (__syncthreads_or(bad)) return;   // a NaN in a selected column: the trajectory's back-offs stay as they are
    for (int k = threadIdx.x; k <= K; k += 64) {
        const bool first = k == 0, last = k == K;
        if (which & SCVX_MARGIN_THRUST) {
            double* m = marg + ((size_t)b * (K + 1) + k) * 2;   // lo alone: |u| is convex along a hold, hi needs nothing between the nodes
            m[0] = fmin(fma(gain, audit_excess(s, K, k, SCVX_SEG_G_TMIN, tol), m[0]), capw.thrust);
        }
        double* pm = pmarg + ((size_t)b * (K + 1) + k) * SCVX_PMARG_N;
        if (which & SCVX_MARGIN_GLIDE) {
            const double width = fmax(x[((size_t)b * (K + 1) + k) * 14 + 1], 0.0) * capw.itan;
            pm[SCVX_PMARG_GLIDE] = first || last ? 0.0 : fmin(fma(gain, audit_excess(s, K, k, SCVX_SEG_G_GLIDE, tol), pm[SCVX_PMARG_GLIDE]),
                                                              capw.cap * width);
        }
        if (which & SCVX_MARGIN_TILT)
            pm[SCVX_PMARG_TILT] = last ? 0.0 : fmin(fma(gain, audit_excess(s, K, k, SCVX_SEG_G_TILT, tol), pm[SCVX_PMARG_TILT]), capw.tilt);
        if (which & SCVX_MARGIN_RATE)
            pm[SCVX_PMARG_RATE] = first || last ? 0.0 : fmin(fma(gain, audit_excess(s, K, k, SCVX_SEG_G_RATE, tol), pm[SCVX_PMARG_RATE]),
                                                             capw.rate);
    }
}

hipError_t launch_segment_audit(const scvx_ctx* ctx, int B, int K, const double* x, const double* u, const double* sigma, int nsub,
                                double* seg, double* report, hipStream_t st) {
    const PathK c = path_constants(ctx->prob);
    const double dt = 1.0 / (K + 1);
    const long nseg = (long)B * K;
    const dim3 g((unsigned)((nseg + 63) / 64)), blk(64);
    const DynP<double> dp(ctx->dyn);
#define SCVX_AUDIT(A, F, T, par) \
    hipLaunchKernelGGL((audit_kernel<A, F, T>), g, blk, 0, st, par, c, nseg, K, x, u, sigma, dt, nsub, seg, report)
    if (ctx->dyn.trq) {
        const DynPT<double> dpt(ctx->dyn);
        if (ctx->dyn.fin) SCVX_AUDIT(true, true, true, dpt);
        else SCVX_AUDIT(true, false, true, dpt);
    } else if (ctx->dyn.fin) {
        if (ctx->dyn.aero) SCVX_AUDIT(true, true, false, dp);
        else SCVX_AUDIT(false, true, false, dp);
    } else if (ctx->dyn.aero)
        SCVX_AUDIT(true, false, false, dp);
    else
        SCVX_AUDIT(false, false, false, dp);
#undef SCVX_AUDIT
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !report) return e;
    hipLaunchKernelGGL(audit_report_kernel, dim3((unsigned)B), blk, 0, st, B, K, seg, report);
    return hipGetLastError();
}

hipError_t launch_audit_margins(int B, int K, const double* seg, const double* x, double gain, double tol, const AuditCaps& capw,
                                unsigned which, double* marg, double* pmarg, hipStream_t st) {
    hipLaunchKernelGGL(audit_margins_kernel, dim3((unsigned)B), dim3(64), 0, st, B, K, seg, x, gain, tol, capw, which, marg, pmarg);
    return hipGetLastError();
}

int check_segment_audit(scvx_ctx* ctx, int B, int K, const void* x, const void* u, const void* sigma, int nsub, const void* seg) {
    if (!ctx) return SCVX_ERR_ARG;
    if (B < 1) return fail(ctx, SCVX_ERR_ARG, "segment audit: B >= 1 required");
    if (K != ctx->prob.K) return fail(ctx, SCVX_ERR_ARG, "segment audit: K must equal the problem's K");
    if (nsub < 1 || nsub > 1000) return fail(ctx, SCVX_ERR_ARG, "segment audit: nsub must be in [1,1000]");
    if (!x || !u || !sigma || !seg) return fail(ctx, SCVX_ERR_ARG, "segment audit: null buffer");
    if (ctx->prob.aero_kind == 1 && !ctx->dyn.aero)
        return fail(ctx, SCVX_ERR_STATE, "AtmosphericData problem: call scvx_set_aero_table first");
    return SCVX_OK;
}

}  // namespace scvx

extern "C" {

int scvx_segment_audit_f64(scvx_ctx* ctx, int B, int K, const double* x_dev, const double* u_dev, const double* sigma_dev, int nsub,
                           double* seg_dev, double* report_dev) {
    if (ctx && nsub == 0) nsub = ctx->nsub;
    int rc = scvx::check_segment_audit(ctx, B, K, x_dev, u_dev, sigma_dev, nsub, seg_dev);
    if (rc) return rc;
    SCVX_HIP(ctx, hipSetDevice(ctx->device));
    SCVX_HIP(ctx, scvx::launch_segment_audit(ctx, B, K, x_dev, u_dev, sigma_dev, nsub, seg_dev, report_dev, ctx->stream));
    return SCVX_OK;
}

int scvx_segment_audit_f64_host(scvx_ctx* ctx, int B, int K, const double* x, const double* u, const double* sigma, int nsub, double* seg,
                                double* report) {
    if (ctx && nsub == 0) nsub = ctx->nsub;
    int rc = scvx::check_segment_audit(ctx, B, K, x, u, sigma, nsub, seg);
    if (rc) return rc;
    const scvx::Dims d(B, K, scvx_control_dim(ctx));
    scvx::Staging s(ctx);
    const double *dx = s.in(x, d.x), *du = s.in(u, d.u), *ds = s.in(sigma, d.b);
    double *dg = s.out(seg, d.aud), *dr = s.out(report, d.frep);
    s.launch([&] { return scvx::launch_segment_audit(ctx, B, K, dx, du, ds, nsub, dg, dr, s.st); });
    return s.finish("scvx_segment_audit_f64_host");
}

}  // extern "C"
